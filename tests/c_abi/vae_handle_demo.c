/* A host program in plain C99 that turns a latent into pixels, and pixels into a latent, through the autoencoder handle of
 * include/vcloze_hip.h - no Python, no torch, no C++: what a caller who has just run vc_flux_sample_ode does next.
 *
 *   vae_handle_demo <in.bin> <out.bin>
 *
 * in.bin (written by tests/test_vae_handle_gpu.py), little endian:
 *   VcVaeConfig | int32 n_weights, h, w
 *   n_weights x { int32 name_len | name | int32 ndim | int64 shape[ndim] | bf16 weight[prod(shape)] | bf16 bias[shape[0]] }
 *   bf16 latent[z_channels][h][w]
 * The tensors are the state_dict entries as stored ([O, I, k, k] convolution weights, [C] GroupNorm affines): the library does the
 * re-layout.  out.bin: bf16 pixels[out_ch][f h][f w] = AutoEncoder.decode(latent) (models/modules/autoencoder.py:306-308), then
 * bf16 latent[z_channels][h][w] = AutoEncoder.encode of those pixels with the distribution's mean (:301-304).
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
  vc_vae_struct_sizes(size);
  if (vc_abi_version() != VC_ABI_VERSION || size[0] != (int32_t)sizeof(VcVaeConfig)) { fprintf(stderr, "library / header mismatch\n"); return 1; }
  VcVaeConfig cfg;
  int32_t head[3];
  rd(&cfg, sizeof(cfg));
  rd(head, sizeof(head));
  const int n_weights = head[0], h = head[1], w = head[2];
  void* handle = NULL;
  CHECK_VC(vc_vae_create(&cfg, &handle));
  hipStream_t stream;
  CHECK_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));

  /* ---- weights, by state_dict key, as stored ---- */
  for (int i = 0; i < n_weights; ++i) {
    char name[160], want[160];
    int32_t len, ndim;
    int64_t shape[4];
    size_t count = 1;
    rd(&len, 4);
    if (len <= 0 || len >= (int32_t)sizeof(name)) { fprintf(stderr, "bad name length\n"); return 1; }
    rd(name, (size_t)len);
    name[len] = 0;
    rd(&ndim, 4);
    if (ndim < 1 || ndim > 4) { fprintf(stderr, "bad ndim\n"); return 1; }
    rd(shape, (size_t)ndim * 8);
    for (int d = 0; d < ndim; ++d) count *= (size_t)shape[d];
    CHECK_VC(vc_vae_weight_name(handle, i, want, (int32_t)sizeof(want)));      /* the file lists them in the handle's order */
    if (strcmp(name, want)) { fprintf(stderr, "weight %d is '%s', the handle expects '%s'\n", i, name, want); return 1; }
    void* dw = to_device(count * 2);
    void* db = to_device((size_t)shape[0] * 2);
    CHECK_VC(vc_vae_bind_weight(handle, name, dw, db, 0, shape, ndim, stream));
    CHECK_HIP(hipFree(dw));                 /* the handle keeps its own re-laid copy */
    CHECK_HIP(hipFree(db));
  }
  char none[8];
  if (vc_vae_weight_name(handle, n_weights, none, (int32_t)sizeof(none)) == VC_OK) { fprintf(stderr, "the handle expects more weights\n"); return 1; }

  /* ---- one image size: workspace for both halves ---- */
  const int f = 1 << (cfg.n_ch_mult - 1), H = f * h, W = f * w;
  int64_t ws_bytes = 0;
  CHECK_VC(vc_vae_workspace_bytes(handle, H, W, VC_VAE_ENCODER | VC_VAE_DECODER, &ws_bytes));
  void* ws = NULL;
  CHECK_HIP(hipMalloc(&ws, (size_t)ws_bytes));
  CHECK_VC(vc_vae_prepare(handle, H, W, VC_VAE_ENCODER | VC_VAE_DECODER, ws, ws_bytes, stream));

  const size_t n_lat = (size_t)cfg.z_channels * h * w, n_pix = (size_t)cfg.out_ch * H * W;
  void* latent = to_device(n_lat * 2);
  void *pixels = NULL, *back = NULL;
  CHECK_HIP(hipMalloc(&pixels, n_pix * 2));
  CHECK_HIP(hipMalloc(&back, n_lat * 2));
  CHECK_VC(vc_vae_decode(handle, latent, VC_VAE_LATENT_BF16, 0, 0, pixels, 0, stream));
  if (cfg.in_channels == cfg.out_ch)
    CHECK_VC(vc_vae_encode(handle, pixels, 0, NULL, back, VC_VAE_LATENT_BF16, 0, 0, stream));
  else
    CHECK_HIP(hipMemsetAsync(back, 0, n_lat * 2, stream));
  CHECK_HIP(hipStreamSynchronize(stream));
  if (vc_vae_plan_count(handle) != (cfg.in_channels == cfg.out_ch ? 2 : 1)) { fprintf(stderr, "unexpected plan count %d\n", vc_vae_plan_count(handle)); return 1; }

  uint16_t* host = (uint16_t*)malloc((n_pix + n_lat) * 2);
  CHECK_HIP(hipMemcpy(host, pixels, n_pix * 2, hipMemcpyDeviceToHost));
  CHECK_HIP(hipMemcpy(host + n_pix, back, n_lat * 2, hipMemcpyDeviceToHost));
  FILE* out = fopen(argv[2], "wb");
  if (!out || fwrite(host, 2, n_pix + n_lat, out) != n_pix + n_lat) { fprintf(stderr, "cannot write %s\n", argv[2]); return 1; }
  fclose(out);
  CHECK_VC(vc_vae_destroy(handle));
  printf("vae_handle_demo: wrote %zu bf16 values\n", n_pix + n_lat);
  return 0;
}
