/* A host program in plain C99 that draws torch's device generator stream from the library - no Python, no torch, no C++: what a
 * caller does who wants the images torch.Generator(device).manual_seed(SEED) gives.
 *
 *   torch_noise_demo
 *
 * One generator, two draws, the offset kept as torch keeps it (vc_torch_randn_policy gives the advance):
 *   1. N1 elements as raw words (VC_RNG_U32) and, at the SAME offset, as F32 normals - the words a restatement must reproduce
 *   2. N2 elements as bf16 at the advanced offset
 * Printed, every word in hex:
 *   policy <n> <grid> <advance>          (once per draw)
 *   u32 <N1 words>
 *   f32 <N1 words>
 *   bf16 <N2 half-words>
 *   offset <the generator's offset after both draws>
 * tests/test_torch_noise_gpu.py makes the same calls through ctypes and compares the text.
 */
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "vcloze_hip.h"

#define CHECK_HIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(2); } } while (0)
#define CHECK_VC(x) do { int rc_ = (x); if (rc_ != 0) { fprintf(stderr, "%s -> %d: %s\n", #x, rc_, vc_last_error()); exit(3); } } while (0)

#define SEED 0x8000000000000001ull
#define OFFSET0 8ull
#define N1 13
#define N2 1030 /* five blocks of 256 threads: every thread's lane 0, nothing further */

int main(void) {
  if (vc_abi_version() != VC_ABI_VERSION) { fprintf(stderr, "library / header mismatch\n"); return 1; }
  uint64_t offset = OFFSET0, advance = 0;
  int32_t grid = 0;
  uint32_t w1[N1], f1[N1];
  uint16_t h2[N2];
  void *a = NULL, *b = NULL, *c = NULL;
  hipStream_t stream;
  CHECK_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
  CHECK_HIP(hipMalloc(&a, N1 * 4));
  CHECK_HIP(hipMalloc(&b, N1 * 4));
  CHECK_HIP(hipMalloc(&c, N2 * 2));

  CHECK_VC(vc_torch_randn_policy(N1, 0, 0, &grid, &advance));
  printf("policy %d %d %llu\n", N1, (int)grid, (unsigned long long)advance);
  CHECK_VC(vc_randn_torch(a, VC_RNG_U32, N1, SEED, offset, 0, 0, stream));
  CHECK_VC(vc_randn_torch(b, VC_RNG_F32, N1, SEED, offset, 0, 0, stream));
  offset += advance;
  CHECK_VC(vc_torch_randn_policy(N2, 0, 0, &grid, &advance));
  printf("policy %d %d %llu\n", N2, (int)grid, (unsigned long long)advance);
  CHECK_VC(vc_randn_torch(c, VC_RNG_BF16, N2, SEED, offset, 0, 0, stream));
  offset += advance;

  /* the argument checks answer on the host, with a message */
  if (vc_randn_torch(a, VC_RNG_U32, N1, SEED, offset + 2, 0, 0, stream) != VC_ERR_ARG || !vc_last_error()[0]) {
    fprintf(stderr, "an offset that is no multiple of 4 accepted\n"); return 1; }
  if (vc_torch_randn_policy(N1, 1, 255, &grid, &advance) != VC_ERR_ARG) { fprintf(stderr, "threads_per_sm 255 accepted\n"); return 1; }

  CHECK_HIP(hipMemcpyAsync(w1, a, N1 * 4, hipMemcpyDeviceToHost, stream));
  CHECK_HIP(hipMemcpyAsync(f1, b, N1 * 4, hipMemcpyDeviceToHost, stream));
  CHECK_HIP(hipMemcpyAsync(h2, c, N2 * 2, hipMemcpyDeviceToHost, stream));
  CHECK_HIP(hipStreamSynchronize(stream));
  printf("u32");
  for (int i = 0; i < N1; ++i) printf(" %08x", (unsigned)w1[i]);
  printf("\nf32");
  for (int i = 0; i < N1; ++i) printf(" %08x", (unsigned)f1[i]);
  printf("\nbf16");
  for (int i = 0; i < N2; ++i) printf(" %04x", (unsigned)h2[i]);
  printf("\noffset %llu\n", (unsigned long long)offset);

  CHECK_HIP(hipFree(a));
  CHECK_HIP(hipFree(b));
  CHECK_HIP(hipFree(c));
  CHECK_HIP(hipStreamDestroy(stream));
  return 0;
}
