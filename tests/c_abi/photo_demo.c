/* A host program in plain C99 that goes from 8-BIT PHOTOGRAPHS to an 8-BIT RESULT through the grid handle of include/vcloze_hip.h:
 * no Python, no torch, no C++, no image library.  It builds the four tiny handles as tests/c_abi/grid_demo.c does, then
 *   vc_grid_layout            the size of the last row
 *   vc_grid_generate_photos   resamples, crop, normalisation, masks and the grid itself; the last row comes back as bytes
 *   (a 2-D copy)              the masked cell's column window of that row
 *   vc_upsampling_size, vc_grid_sdedit_u8   the cell resized on the device and refined; the result as bytes
 *
 *   photo_demo <in.bin> <out.bin>
 *
 * in.bin (written by tests/test_photo_handle_gpu.py): the four handles exactly as grid_demo.c reads them, then
 *   int32 grid_h, grid_w, resolution | grid_h * grid_w x { int32 H, W (0, 0 = absent) | uint8 pixels[H][W][3] }
 *   int32 t5_len | int32 ids[t5_len] | int32 clip_len | int32 ids[clip_len]
 *   uint64 seed, noise_offset | float guidance | int32 n_points, method | double time_shifting_factor
 *   int32 target_w, target_h (0, 0 = none), upsampling n_points | double strength
 * out.bin: int32 h, w | uint8 [h][w][3], the refined cell | the uint64 stream position behind the last draw.
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
  vc_photo_struct_sizes(gs);
  if (vc_abi_version() != VC_ABI_VERSION || gs[0] != (int32_t)sizeof(VcCellPlan) || gs[1] != (int32_t)sizeof(VcGridPhotos) ||
      gs[2] != (int32_t)sizeof(VcGridSdeditU8)) {
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

  /* ---- the photographs ---- */
  VcGridPhotos job;
  memset(&job, 0, sizeof(job));
  job.grid_h = rd_i32();
  job.grid_w = rd_i32();
  job.resolution = rd_i32();
  if (job.grid_h < 1 || job.grid_h > VC_GRID_MAX_ROWS || job.grid_w < 1 || job.grid_w > VC_GRID_MAX_ROWS) { fprintf(stderr, "bad grid\n"); return 1; }
  const int cells = job.grid_h * job.grid_w;
  const void* images[VC_GRID_MAX_ROWS * VC_GRID_MAX_ROWS] = {0};
  int32_t widths[VC_GRID_MAX_ROWS * VC_GRID_MAX_ROWS] = {0}, heights[VC_GRID_MAX_ROWS * VC_GRID_MAX_ROWS] = {0};
  for (int c = 0; c < cells; ++c) {
    heights[c] = rd_i32();
    widths[c] = rd_i32();
    if (heights[c] > 0 && widths[c] > 0) images[c] = to_device((size_t)heights[c] * widths[c] * 3);
  }
  job.images = images;
  job.width = widths;
  job.height = heights;
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
  job.out_form = VC_PIXELS_U8;
  job.noise_offset_out = &after;
  const int32_t target_w = rd_i32(), target_h = rd_i32(), up_points = rd_i32();
  double strength;
  rd(&strength, 8);

  /* the last row's size, and its first masked cell */
  VcCellPlan plan[VC_GRID_MAX_ROWS * VC_GRID_MAX_ROWS];
  CHECK_VC(vc_grid_layout(job.grid_h, job.grid_w, widths, heights, job.resolution, plan));
  const VcCellPlan* last = plan + (job.grid_h - 1) * job.grid_w;
  int32_t row_w = 0, cell_x0 = -1, cell_w = 0;
  const int32_t row_h = last[0].final_h;
  for (int k = 0; k < job.grid_w; ++k) {
    if (last[k].mask && cell_x0 < 0) { cell_x0 = row_w; cell_w = last[k].final_w; }
    row_w += last[k].final_w;
  }
  if (cell_x0 < 0) { fprintf(stderr, "no cell to generate\n"); return 1; }
  void* out_rows[VC_GRID_MAX_ROWS] = {0};
  job.decode[job.grid_h - 1] = 1;
  CHECK_HIP(hipMalloc(&out_rows[job.grid_h - 1], (size_t)row_h * row_w * 3));

  int64_t ws_bytes = 0;
  CHECK_VC(vc_grid_photos_workspace_bytes(grid, &job, &ws_bytes));
  void* ws = NULL;
  CHECK_HIP(hipMalloc(&ws, (size_t)ws_bytes));
  CHECK_VC(vc_grid_generate_photos(grid, &job, ws, ws_bytes, out_rows, stream));

  /* the cell: columns [cell_x0, cell_x0 + cell_w) of the 8-bit row, made dense */
  void* cell = NULL;
  CHECK_HIP(hipMalloc(&cell, (size_t)row_h * cell_w * 3));
  CHECK_HIP(hipMemcpy2DAsync(cell, (size_t)cell_w * 3, (const unsigned char*)out_rows[job.grid_h - 1] + (size_t)cell_x0 * 3, (size_t)row_w * 3,
                             (size_t)cell_w * 3, (size_t)row_h, hipMemcpyDeviceToDevice, stream));

  VcGridSdeditU8 up;
  memset(&up, 0, sizeof(up));
  up.count = 1;
  up.cell_h = row_h;
  up.cell_w = cell_w;
  CHECK_VC(vc_upsampling_size(target_w, target_h, &up.width, &up.height));
  up.out_form = VC_PIXELS_U8;
  up.pixels[0] = cell;
  up.t5_ids = t5_ids; up.clip_ids = clip_ids; up.t5_len = job.t5_len; up.clip_len = job.clip_len;
  up.seed = job.seed;
  up.noise_offset = after;                 /* the second stage goes on drawing where the first stopped */
  up.noise_offset_out = &after;
  up.guidance = job.guidance; up.n_points = up_points; up.method = job.method;
  up.strength = strength;
  void* result = NULL;
  const size_t result_bytes = (size_t)up.height * up.width * 3;
  CHECK_HIP(hipMalloc(&result, result_bytes));
  int64_t ws2_bytes = 0;
  CHECK_VC(vc_grid_sdedit_u8_workspace_bytes(grid, &up, &ws2_bytes));
  void* ws2 = NULL;
  CHECK_HIP(hipMalloc(&ws2, (size_t)ws2_bytes));
  void* outs[1] = {result};
  CHECK_VC(vc_grid_sdedit_u8(grid, &up, ws2, ws2_bytes, outs, stream));
  CHECK_HIP(hipStreamSynchronize(stream));

  unsigned char* host = (unsigned char*)malloc(result_bytes);
  CHECK_HIP(hipMemcpy(host, result, result_bytes, hipMemcpyDeviceToHost));
  FILE* out = fopen(argv[2], "wb");
  const int32_t hw[2] = {up.height, up.width};
  if (!out || fwrite(hw, 4, 2, out) != 2 || fwrite(host, 1, result_bytes, out) != result_bytes || fwrite(&after, 8, 1, out) != 1) {
    fprintf(stderr, "cannot write %s\n", argv[2]);
    return 1;
  }
  fclose(out);
  CHECK_VC(vc_grid_destroy(grid));       /* the sub-handles are ours */
  CHECK_VC(vc_flux_destroy(gc.flux));
  CHECK_VC(vc_vae_destroy(gc.vae));
  CHECK_VC(vc_text_destroy(gc.t5));
  CHECK_VC(vc_text_destroy(gc.clip));
  printf("photo_demo: wrote %dx%d pixels, stream position %llu\n", up.width, up.height, (unsigned long long)after);
  return 0;
}
