/* flux_handle_demo.c once more, fed as a CHECKPOINT: a host program in plain C99 that hands the library the tensors of a
 * FLUX + LoRA state_dict as they are stored - qkv rows in their natural order, every modulation Linear on its own, a rank-16
 * LoRA pair on every Linear but one (txt_in) - and lets vc_flux_load_* merge (scale 0.75), permute, stack, cast and bind them.
 *
 *   flux_load_demo <out.bin>
 *
 * The keys and shapes come from vc_flux_load_key; the values are the procedural ones of flux_handle_demo.c (value formula below =
 * tests/test_c_abi.py::fill), named by their state_dict key.  One vc_flux_forward and a 4-step Euler trajectory follow, written as
 * forward [24 x 64] | final state [24 x 64] | trajectory [4 x 24 x 64], raw bf16.  tests/test_flux_load_gpu.py compares the file bit
 * for bit with the same calls made from Python over the same tensors.
 */
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "vcloze_hip.h"

enum { IN_CH = 384, OUT_CH = 64, VEC = 64, CTX = 128, D = 256, HEADS = 2, DEPTH = 2, SINGLE = 2, MLP = 1024, T = 16, N = 24, STEPS = 4, RANK = 16 };

#define CHECK_HIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(2); } } while (0)
#define CHECK_VC(x) do { int rc_ = (x); if (rc_ != 0) { fprintf(stderr, "%s -> %d: %s\n", #x, rc_, vc_last_error()); exit(3); } } while (0)

/* value k of tensor `seed`: an LCG word -> [-1, 1) -> * scale -> bf16 (round to nearest even) */
static uint16_t bf16_bits(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
static uint16_t value(uint32_t seed, uint32_t k, float scale) {
  const uint32_t w = seed * 1664525u + k * 1013904223u + 12345u;
  const float f = ((float)(int32_t)(w >> 16) - 32768.0f) * (1.0f / 32768.0f);
  return bf16_bits(f * scale);
}
static uint32_t name_seed(const char* s) {   /* FNV-1a */
  uint32_t h = 2166136261u;
  for (; *s; ++s) { h ^= (uint8_t)*s; h *= 16777619u; }
  return h;
}
static void* dev_fill(const char* name, size_t count, float scale, float offset) {
  uint16_t* h = (uint16_t*)malloc(count * 2);
  const uint32_t seed = name_seed(name);
  for (size_t k = 0; k < count; ++k) {
    uint16_t b = value(seed, (uint32_t)k, scale);
    if (offset != 0.0f) { uint32_t u = (uint32_t)b << 16; float f; memcpy(&f, &u, 4); b = bf16_bits(f + offset); }
    h[k] = b;
  }
  void* d = NULL;
  CHECK_HIP(hipMalloc(&d, count * 2));
  CHECK_HIP(hipMemcpy(d, h, count * 2, hipMemcpyHostToDevice));
  free(h);
  return d;
}
static int ends_with(const char* s, const char* tail) {
  const size_t n = strlen(s), m = strlen(tail);
  return n >= m && !strcmp(s + n - m, tail);
}

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s out.bin\n", argv[0]); return 1; }
  int32_t sizes[7];
  vc_struct_sizes(sizes);
  if (vc_abi_version() != VC_ABI_VERSION || sizes[4] != (int32_t)sizeof(VcFluxConfig) || sizes[5] != (int32_t)sizeof(VcFluxInputs)) {
    fprintf(stderr, "library / header mismatch\n");
    return 1;
  }
  void* handle = NULL;
  VcFluxConfig cfg = {IN_CH, OUT_CH, VEC, CTX, D, HEADS, DEPTH, SINGLE, MLP, 1, {16, 56, 56}, 10000};
  CHECK_VC(vc_flux_create(&cfg, &handle));

  /* ---- the checkpoint: every key the library lists, as stored ---- */
  char key[160];
  int64_t shape[2];
  int32_t ndim, n_keys = 0, n_recorded = 0;
  for (; vc_flux_load_key(handle, n_keys, key, (int32_t)sizeof(key), shape, &ndim) == VC_OK; ++n_keys) {
    if (!strncmp(key, "txt_in.lora_", 12)) continue;             /* one Linear without a pair */
    size_t count = 1;
    for (int d = 0; d < ndim; ++d) { if (shape[d] < 0) shape[d] = RANK; count *= (size_t)shape[d]; }
    float scale = 0.06f, offset = 0.0f;
    if (ends_with(key, ".scale")) { scale = 0.1f; offset = 1.0f; }           /* QKNorm scales around 1 */
    else if (ends_with(key, ".lora_A.weight") || ends_with(key, ".lora_B.weight")) scale = 0.1f;
    else if (ends_with(key, ".lora_B.bias")) scale = 0.02f;
    else if (ends_with(key, ".bias")) scale = 0.05f;
    CHECK_VC(vc_flux_load_tensor(handle, key, dev_fill(key, count, scale, offset), 0, shape, ndim));
    ++n_recorded;
  }
  hipStream_t stream;
  CHECK_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
  const int64_t arena_bytes = vc_flux_load_bytes(handle);
  void* arena = NULL;
  CHECK_HIP(hipMalloc(&arena, (size_t)arena_bytes));
  CHECK_VC(vc_flux_load_finish(handle, 0.75f, arena, arena_bytes, stream));
  const void* w = NULL;
  int32_t rows = 0, cols = 0;
  CHECK_VC(vc_flux_bound(handle, "modulation", &w, NULL, &rows, &cols, NULL));
  if (rows != vc_flux_mod_offset(handle, NULL) || cols != D || (const char*)w < (const char*)arena || (const char*)w >= (const char*)arena + arena_bytes) {
    fprintf(stderr, "unexpected modulation binding\n");
    return 1;
  }

  /* ---- one sample ---- */
  void* txt = dev_fill("input.txt", (size_t)T * CTX, 1.0f, 0.0f);
  void* y = dev_fill("input.y", VEC, 1.0f, 0.0f);
  void* x = dev_fill("input.x", (size_t)N * OUT_CH, 1.0f, 0.0f);
  void* cond = dev_fill("input.cond", (size_t)N * (IN_CH - OUT_CH), 1.0f, 0.0f);
  float img_ids[N * 3], txt_ids[T * 3], guidance[1] = {30.0f};
  memset(txt_ids, 0, sizeof(txt_ids));
  for (int r = 0; r < N; ++r) {            /* two grid rows of 2 x 6 tokens: (row index + 1, y, x), models/sampling.py:47-60 */
    img_ids[3 * r] = (float)(r / 12 + 1);
    img_ids[3 * r + 1] = (float)((r % 12) / 6);
    img_ids[3 * r + 2] = (float)(r % 6);
  }
  const int64_t ws_bytes = vc_flux_workspace_bytes(handle, 1, T, N, STEPS);
  void* ws = NULL;
  CHECK_HIP(hipMalloc(&ws, (size_t)ws_bytes));
  VcFluxInputs in;
  memset(&in, 0, sizeof(in));
  in.B = 1; in.T = T; in.N = N; in.max_steps = STEPS;
  in.txt = txt; in.y = y; in.guidance = guidance; in.img_ids = img_ids; in.txt_ids = txt_ids;
  CHECK_VC(vc_flux_prepare(handle, &in, ws, ws_bytes, stream));

  /* ---- Flux.forward: one evaluation of x || cond at t = 0.7 ---- */
  void *img = NULL, *fwd = NULL, *traj = NULL;
  CHECK_HIP(hipMalloc(&img, (size_t)N * IN_CH * 2));
  CHECK_HIP(hipMalloc(&fwd, (size_t)N * OUT_CH * 2));
  CHECK_HIP(hipMalloc(&traj, (size_t)STEPS * N * OUT_CH * 2));
  CHECK_VC(vc_concat_cols(x, OUT_CH, cond, IN_CH - OUT_CH, img, N, stream));
  const float t07[1] = {0.7f};
  CHECK_VC(vc_flux_forward(handle, img, t07, 0, fwd, stream));

  /* ---- the Euler loop: 5 solver points from 0 to 1, bf16 state, x updated in place ---- */
  const float grid[STEPS + 1] = {0.0f, 0.25f, 0.5f, 0.75f, 1.0f};
  CHECK_VC(vc_flux_sample_euler(handle, x, cond, grid, STEPS + 1, 1, traj, stream));
  CHECK_HIP(hipStreamSynchronize(stream));

  uint16_t* host = (uint16_t*)malloc((size_t)(2 + STEPS) * N * OUT_CH * 2);
  CHECK_HIP(hipMemcpy(host, fwd, (size_t)N * OUT_CH * 2, hipMemcpyDeviceToHost));
  CHECK_HIP(hipMemcpy(host + N * OUT_CH, x, (size_t)N * OUT_CH * 2, hipMemcpyDeviceToHost));
  CHECK_HIP(hipMemcpy(host + 2 * N * OUT_CH, traj, (size_t)STEPS * N * OUT_CH * 2, hipMemcpyDeviceToHost));
  FILE* f = fopen(argv[1], "wb");
  if (!f || fwrite(host, 2, (size_t)(2 + STEPS) * N * OUT_CH, f) != (size_t)(2 + STEPS) * N * OUT_CH) { fprintf(stderr, "cannot write %s\n", argv[1]); return 1; }
  fclose(f);
  CHECK_VC(vc_flux_destroy(handle));
  printf("flux_load_demo: %d of %d keys recorded, wrote %d bf16 values\n", n_recorded, n_keys, (2 + STEPS) * N * OUT_CH);
  return 0;
}
