/* A host program in plain C99 that draws the two kinds of noise a generation needs from the library's own stream - no Python, no
 * torch, no C++: what a caller of vc_vae_encode and vc_flux_sample_ode does for their `noise` and x(t0) operands.
 *
 *   noise_demo
 *
 * With one seed and one running stream offset, as pipeline.NoiseStream keeps them:
 *   1. the DiagonalGaussian draw of an encode: vc_randn, bf16 [Z][H][W] at offset OFFSET0
 *   2. the sampler's start state: vc_randn_tokens, the next Z*H*W positions, straight into columns COL0 .. COL0 + 4 Z of
 *      (H/2)(W/2) token rows of LD elements (the rest of the rows, zeroed here, is the caller's `cond`)
 * Both are copied back and their 64-bit FNV-1a hashes printed:
 *   encode_noise <hex>
 *   tokens <hex>
 * tests/test_noise_gpu.py makes the same two calls through ctypes and compares the hashes.
 */
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "vcloze_hip.h"

#define CHECK_HIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(2); } } while (0)
#define CHECK_VC(x) do { int rc_ = (x); if (rc_ != 0) { fprintf(stderr, "%s -> %d: %s\n", #x, rc_, vc_last_error()); exit(3); } } while (0)

#define SEED 0x0123456789ABCDEFull
#define OFFSET0 17179869179ull /* 2^34 - 5: the first draw crosses the carry of the block counter into its second word */
#define Z 16
#define H 6
#define W 10
#define LD 128
#define COL0 64

static uint64_t fnv64(const unsigned char* p, size_t n) {
  uint64_t h = 0xCBF29CE484222325ull;
  for (size_t i = 0; i < n; ++i) h = (h ^ p[i]) * 0x100000001B3ull;
  return h;
}

int main(void) {
  if (vc_abi_version() != VC_ABI_VERSION) { fprintf(stderr, "library / header mismatch\n"); return 1; }
  const size_t n = (size_t)Z * H * W, tok_elems = (size_t)(H / 2) * (W / 2) * LD;
  uint64_t offset = OFFSET0;
  void *noise = NULL, *tokens = NULL;
  hipStream_t stream;
  CHECK_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
  CHECK_HIP(hipMalloc(&noise, n * 2));
  CHECK_HIP(hipMalloc(&tokens, tok_elems * 2));
  CHECK_HIP(hipMemsetAsync(tokens, 0, tok_elems * 2, stream));

  CHECK_VC(vc_randn(noise, VC_RNG_BF16, (int64_t)n, SEED, offset, stream));
  offset += n;
  CHECK_VC(vc_randn_tokens(tokens, Z, H, W, LD, COL0, SEED, offset, stream));
  offset += n;

  /* the argument checks answer on the host, with a message */
  if (vc_randn(noise, 7, (int64_t)n, SEED, offset, stream) != VC_ERR_ARG || !vc_last_error()[0]) { fprintf(stderr, "dtype 7 accepted\n"); return 1; }
  if (vc_randn_tokens(tokens, Z, H + 1, W, LD, COL0, SEED, offset, stream) != VC_ERR_ARG) { fprintf(stderr, "odd h accepted\n"); return 1; }

  unsigned char* host = (unsigned char*)malloc(tok_elems * 2 > n * 2 ? tok_elems * 2 : n * 2);
  if (!host) return 1;
  CHECK_HIP(hipMemcpyAsync(host, noise, n * 2, hipMemcpyDeviceToHost, stream));
  CHECK_HIP(hipStreamSynchronize(stream));
  printf("encode_noise %016llx\n", (unsigned long long)fnv64(host, n * 2));
  CHECK_HIP(hipMemcpyAsync(host, tokens, tok_elems * 2, hipMemcpyDeviceToHost, stream));
  CHECK_HIP(hipStreamSynchronize(stream));
  printf("tokens %016llx\n", (unsigned long long)fnv64(host, tok_elems * 2));

  free(host);
  CHECK_HIP(hipFree(noise));
  CHECK_HIP(hipFree(tokens));
  CHECK_HIP(hipStreamDestroy(stream));
  return 0;
}
