/* A host program in plain C99 that generates ONE GRID - pixels and token ids in, pixels out - through the grid handle of
 * include/vcloze_hip.h: no Python, no torch, no C++.  It builds the four tiny handles (Flux, autoencoder, T5, CLIP) from the
 * procedural weights its input file carries, hands them to vc_grid_create and makes one vc_grid_generate call; the time grid, the
 * img_ids, the order of the noise draws and the pixel epilogue are the library's.
 *
 *   grid_demo <in.bin> <out.bin>
 *
 * in.bin (written by tests/test_grid_demo_gpu.py), little endian; a `tensor` is
 *   int32 name_len | name | int32 ndim | int64 shape[ndim] | int32 elem_bytes | data | int32 has_bias | bias[shape[0]] (same element size)
 * and the file is
 *   VcFluxConfig | int32 n_options x { int32 name_len | name | int32 value } | int32 n x tensor     (2-D weights, [128] scales, "modulation",
 *                                                                                                    "timestep_freqs" as F32)
 *   VcVaeConfig  | int32 n x tensor            (state_dict entries as stored, each with its bias)
 *   VcTextConfig | int32 n x tensor            (T5: every state_dict key, no biases)
 *   VcTextConfig | int32 n x tensor            (CLIP)
 *   int32 rows | rows x { int32 H, W | bf16 pixels[3][H][W] | bf16 mask[H][W] | int32 decode }
 *   int32 t5_len | int32 ids[t5_len] | int32 clip_len | int32 ids[clip_len]
 *   uint64 seed, noise_offset | float guidance | int32 n_points, method | double time_shifting_factor
 * out.bin: per decoded row F32 [3][H][W] in [0, 1], then the uint64 stream position behind the last draw.
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
static int32_t rd_i32(void) { int32_t v; rd(&v, 4); return v; }
static void rd_name(char* name, size_t cap) {
  const int32_t len = rd_i32();
  if (len <= 0 || (size_t)len >= cap) { fprintf(stderr, "bad name length\n"); exit(1); }
  rd(name, (size_t)len);
  name[len] = 0;
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

typedef struct Tensor { char name[160]; int32_t ndim, elem; int64_t shape[4]; void *w, *b; } Tensor;
static void rd_tensor(Tensor* t) {
  size_t count = 1;
  rd_name(t->name, sizeof(t->name));
  t->ndim = rd_i32();
  if (t->ndim < 1 || t->ndim > 4) { fprintf(stderr, "bad ndim\n"); exit(1); }
  rd(t->shape, (size_t)t->ndim * 8);
  for (int d = 0; d < t->ndim; ++d) count *= (size_t)t->shape[d];
  t->elem = rd_i32();
  t->w = to_device(count * (size_t)t->elem);
  t->b = rd_i32() ? to_device((size_t)t->shape[0] * (size_t)t->elem) : NULL;
}

int main(int argc, char** argv) {
  if (argc < 3) { fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 1; }
  in = fopen(argv[1], "rb");
  if (!in) { fprintf(stderr, "cannot read %s\n", argv[1]); return 1; }
  int32_t gs[3];
  vc_grid_struct_sizes(gs);
  if (vc_abi_version() != VC_ABI_VERSION || gs[0] != (int32_t)sizeof(VcGridConfig) || gs[1] != (int32_t)sizeof(VcGridJob) ||
      gs[2] != (int32_t)sizeof(VcGridSdedit)) {
    fprintf(stderr, "library / header mismatch\n");
    return 1;
  }
  hipStream_t stream;
  CHECK_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
  VcGridConfig gc;
  Tensor t;
  char name[160];

  /* ---- Flux: options, then the weights by reference module path ---- */
  VcFluxConfig fc;
  rd(&fc, sizeof(fc));
  CHECK_VC(vc_flux_create(&fc, &gc.flux));
  for (int32_t i = 0, n = rd_i32(); i < n; ++i) {
    rd_name(name, sizeof(name));
    CHECK_VC(vc_flux_set_option(gc.flux, name, rd_i32()));
  }
  for (int32_t i = 0, n = rd_i32(); i < n; ++i) {
    rd_tensor(&t);
    const int32_t rows = t.ndim == 2 ? (int32_t)t.shape[0] : 1, cols = (int32_t)t.shape[t.ndim - 1];
    CHECK_VC(vc_flux_bind_weight(gc.flux, t.name, t.w, t.b, rows, cols, cols));      /* bound by pointer: kept */
  }

  /* ---- autoencoder: the state dict as stored; the handle keeps its own re-laid copies ---- */
  VcVaeConfig vcfg;
  rd(&vcfg, sizeof(vcfg));
  CHECK_VC(vc_vae_create(&vcfg, &gc.vae));
  for (int32_t i = 0, n = rd_i32(); i < n; ++i) {
    rd_tensor(&t);
    CHECK_VC(vc_vae_bind_weight(gc.vae, t.name, t.w, t.b, t.elem == 4, t.shape, t.ndim, stream));
    CHECK_HIP(hipFree(t.w));
    CHECK_HIP(hipFree(t.b));
  }

  /* ---- T5 and CLIP: every state_dict key, bound by pointer ---- */
  for (int which = 0; which < 2; ++which) {
    VcTextConfig tc;
    void** h = which ? &gc.clip : &gc.t5;
    rd(&tc, sizeof(tc));
    CHECK_VC(vc_text_create(&tc, h));
    for (int32_t i = 0, n = rd_i32(); i < n; ++i) {
      rd_tensor(&t);
      CHECK_VC(vc_text_bind_tensor(*h, t.name, t.w, t.shape, t.ndim));
    }
  }

  void* grid = NULL;
  CHECK_VC(vc_grid_create(&gc, &grid));

  /* ---- the job ---- */
  VcGridJob job;
  memset(&job, 0, sizeof(job));
  job.rows = rd_i32();
  if (job.rows < 1 || job.rows > VC_GRID_MAX_ROWS) { fprintf(stderr, "bad row count\n"); return 1; }
  void* out_rows[VC_GRID_MAX_ROWS] = {0};
  size_t out_floats = 0;
  for (int i = 0; i < job.rows; ++i) {
    const int32_t H = rd_i32(), W = rd_i32();
    job.height[i] = H;
    job.width[i] = W;
    job.pixels[i] = to_device((size_t)3 * H * W * 2);
    job.masks[i] = to_device((size_t)H * W * 2);
    job.decode[i] = rd_i32();
    if (job.decode[i]) {
      CHECK_HIP(hipMalloc(&out_rows[i], (size_t)3 * H * W * 4));
      out_floats += (size_t)3 * H * W;
    }
  }
  job.t5_len = rd_i32();
  int32_t* t5_ids = (int32_t*)malloc((size_t)job.t5_len * 4);
  rd(t5_ids, (size_t)job.t5_len * 4);
  job.clip_len = rd_i32();
  int32_t* clip_ids = (int32_t*)malloc((size_t)job.clip_len * 4);
  rd(clip_ids, (size_t)job.clip_len * 4);
  job.t5_ids = t5_ids;
  job.clip_ids = clip_ids;
  uint64_t after = 0;
  rd(&job.seed, 8);
  rd(&job.noise_offset, 8);
  rd(&job.guidance, 4);
  job.n_points = rd_i32();
  job.method = rd_i32();
  rd(&job.time_shifting_factor, 8);
  job.out_form = VC_PIXELS_F32;
  job.noise_offset_out = &after;

  int64_t ws_bytes = 0;
  CHECK_VC(vc_grid_workspace_bytes(grid, &job, &ws_bytes));
  void* ws = NULL;
  CHECK_HIP(hipMalloc(&ws, (size_t)ws_bytes));
  CHECK_VC(vc_grid_generate(grid, &job, ws, ws_bytes, out_rows, stream));
  const int vae_plans = vc_vae_plan_count(gc.vae), t5_plans = vc_text_plan_count(gc.t5);
  CHECK_VC(vc_grid_generate(grid, &job, ws, ws_bytes, out_rows, stream));      /* the same geometry again: every plan serves */
  CHECK_HIP(hipStreamSynchronize(stream));
  if (vc_vae_plan_count(gc.vae) != vae_plans || vc_text_plan_count(gc.t5) != t5_plans || vae_plans < 1 || t5_plans != 1) {
    fprintf(stderr, "unexpected plan counts %d / %d\n", vc_vae_plan_count(gc.vae), vc_text_plan_count(gc.t5));
    return 1;
  }

  float* host = (float*)malloc(out_floats * 4);
  size_t off = 0;
  for (int i = 0; i < job.rows; ++i) {
    if (!job.decode[i]) continue;
    const size_t n = (size_t)3 * job.height[i] * job.width[i];
    CHECK_HIP(hipMemcpy(host + off, out_rows[i], n * 4, hipMemcpyDeviceToHost));
    off += n;
  }
  FILE* out = fopen(argv[2], "wb");
  if (!out || fwrite(host, 4, out_floats, out) != out_floats || fwrite(&after, 8, 1, out) != 1) { fprintf(stderr, "cannot write %s\n", argv[2]); return 1; }
  fclose(out);
  CHECK_VC(vc_grid_destroy(grid));       /* the sub-handles are ours */
  CHECK_VC(vc_flux_destroy(gc.flux));
  CHECK_VC(vc_vae_destroy(gc.vae));
  CHECK_VC(vc_text_destroy(gc.t5));
  CHECK_VC(vc_text_destroy(gc.clip));
  printf("grid_demo: wrote %zu f32 values, stream position %llu\n", out_floats, (unsigned long long)after);
  return 0;
}
