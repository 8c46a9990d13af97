/* A host program in plain C99 that turns token ids into the two text inputs of vc_flux_prepare - VcFluxInputs.txt (T5's
 * last_hidden_state) or VcFluxInputs.y (CLIP's pooler_output) - through the text-encoder handle of include/vcloze_hip.h: no Python,
 * no torch, no C++.  What a caller does before vc_flux_prepare (HFEmbedder.forward, models/modules/conditioner.py:5-37).
 *
 *   text_handle_demo <in.bin> <out.bin>
 *
 * in.bin (written by tests/test_text_handle_gpu.py), little endian:
 *   VcTextConfig | int32 n_tensors, n_prompts, L
 *   n_tensors x { int32 key_len | key | int32 ndim | int64 shape[ndim] | bf16 data[prod(shape)] }
 *   int32 ids[n_prompts][L]
 * The tensors are the state_dict entries as stored, in the handle's order; they are bound by pointer and stay allocated.
 * out.bin: bf16 hidden[n_prompts][L][d_model], then - CLIP only - bf16 pooled[n_prompts][d_model].
 */
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "vcloze_hip.h"

#define CHECK_HIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(2); } } while (0)
#define CHECK_VC(x) do { int rc_ = (x); if (rc_ != 0) { fprintf(stderr, "%s -> %d: %s\n", #x, rc_, vc_last_error()); exit(3); } } while (0)

static FILE* in;
static void rd(void* p, size_t n) {
  if (fread(p, 1, n, in) != n) { fprintf(stderr, "input file too short\n"); exit(1); }
}
static void* to_device(size_t bytes) {      /* the next `bytes` of the file, in device memory */
  void* h = malloc(bytes);
  void* d = NULL;
  rd(h, bytes);
  CHECK_HIP(hipMalloc(&d, bytes));
  CHECK_HIP(hipMemcpy(d, h, bytes, hipMemcpyHostToDevice));
  free(h);
  return d;
}

int main(int argc, char** argv) {
  if (argc < 3) { fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 1; }
  in = fopen(argv[1], "rb");
  if (!in) { fprintf(stderr, "cannot read %s\n", argv[1]); return 1; }
  int32_t size[1];
  vc_text_struct_sizes(size);
  if (vc_abi_version() != VC_ABI_VERSION || size[0] != (int32_t)sizeof(VcTextConfig)) { fprintf(stderr, "library / header mismatch\n"); return 1; }
  VcTextConfig cfg;
  int32_t head[3];
  rd(&cfg, sizeof(cfg));
  rd(head, sizeof(head));
  const int n_tensors = head[0], n_prompts = head[1], L = head[2];
  const int clip = cfg.kind == VC_TEXT_CLIP;
  void* handle = NULL;
  CHECK_VC(vc_text_create(&cfg, &handle));
  hipStream_t stream;
  CHECK_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));

  /* ---- tensors, by state_dict key, as stored: bound by pointer, so they stay allocated ---- */
  for (int i = 0; i < n_tensors; ++i) {
    char key[160], want[160];
    int32_t len, ndim;
    int64_t shape[2];
    size_t count = 1;
    rd(&len, 4);
    if (len <= 0 || len >= (int32_t)sizeof(key)) { fprintf(stderr, "bad key length\n"); return 1; }
    rd(key, (size_t)len);
    key[len] = 0;
    rd(&ndim, 4);
    if (ndim < 1 || ndim > 2) { fprintf(stderr, "bad ndim\n"); return 1; }
    rd(shape, (size_t)ndim * 8);
    for (int d = 0; d < ndim; ++d) count *= (size_t)shape[d];
    CHECK_VC(vc_text_weight_name(handle, i, want, (int32_t)sizeof(want)));      /* the file lists them in the handle's order */
    if (strcmp(key, want)) { fprintf(stderr, "tensor %d is '%s', the handle expects '%s'\n", i, key, want); return 1; }
    CHECK_VC(vc_text_bind_tensor(handle, key, to_device(count * 2), shape, ndim));
  }
  char none[8];
  if (vc_text_weight_name(handle, n_tensors, none, (int32_t)sizeof(none)) == VC_OK) { fprintf(stderr, "the handle expects more tensors\n"); return 1; }

  /* ---- one sequence length: workspace, prepare, every prompt in one call ---- */
  int64_t ws_bytes = 0;
  CHECK_VC(vc_text_workspace_bytes(handle, L, &ws_bytes));
  void* ws = NULL;
  CHECK_HIP(hipMalloc(&ws, (size_t)ws_bytes));
  CHECK_VC(vc_text_prepare(handle, L, ws, ws_bytes, stream));

  const size_t n_hid = (size_t)n_prompts * L * cfg.d_model, n_pool = clip ? (size_t)n_prompts * cfg.d_model : 0;
  int32_t* ids = (int32_t*)to_device((size_t)n_prompts * L * 4);
  void *hidden = NULL, *pooled = NULL;
  CHECK_HIP(hipMalloc(&hidden, n_hid * 2));
  if (clip) CHECK_HIP(hipMalloc(&pooled, n_pool * 2));
  CHECK_VC(vc_text_encode(handle, ids, n_prompts, hidden, pooled, stream));
  CHECK_HIP(hipStreamSynchronize(stream));
  if (vc_text_plan_count(handle) != 1) { fprintf(stderr, "unexpected plan count %d\n", vc_text_plan_count(handle)); return 1; }

  uint16_t* host = (uint16_t*)malloc((n_hid + n_pool) * 2 + 2);
  CHECK_HIP(hipMemcpy(host, hidden, n_hid * 2, hipMemcpyDeviceToHost));
  if (clip) CHECK_HIP(hipMemcpy(host + n_hid, pooled, n_pool * 2, hipMemcpyDeviceToHost));
  FILE* out = fopen(argv[2], "wb");
  if (!out || fwrite(host, 2, n_hid + n_pool, out) != n_hid + n_pool) { fprintf(stderr, "cannot write %s\n", argv[2]); return 1; }
  fclose(out);
  CHECK_VC(vc_text_destroy(handle));
  printf("text_handle_demo: wrote %zu bf16 values\n", n_hid + n_pool);
  return 0;
}
