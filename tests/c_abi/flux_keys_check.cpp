// csrc/flux_keys.h + flux_keys.hip on the host, alone: the state_dict key table and shape parser behind vc_flux_load_key /
// vc_flux_load_tensor / vc_flux_load_bytes.  Built and run by tests/test_flux_load_cpu.py with -Wall -Werror
// -fsanitize=address,undefined; exit status 0 and "flux_keys ok" = every check held.
#include "flux_keys.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>

#define CHECK(cond)                                                              \
  do {                                                                           \
    if (!(cond)) {                                                               \
      fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond);   \
      exit(1);                                                                   \
    }                                                                            \
  } while (0)

static int64_t c256(int64_t v) { return (v + 255) / 256 * 256; }

static void check(const VcFluxConfig& cfg) {
  const vckeys::Table t = vckeys::build(cfg);
  const int D = cfg.hidden_size;
  const int linears = 5 + 2 * (cfg.guidance_embed ? 1 : 0) + 1 + 10 * cfg.depth + 3 * cfg.depth_single_blocks + 2;
  const int scales = 4 * cfg.depth + 2 * cfg.depth_single_blocks;
  CHECK((int)t.linears.size() == linears && (int)t.scales.size() == scales && (int)t.keys.size() == 5 * linears + scales);
  CHECK(t.n_mod == (int64_t)cfg.depth * 12 * D + (int64_t)cfg.depth_single_blocks * 3 * D + 2 * D);
  char err[256] = "";
  std::set<std::string> seen;
  int64_t bytes = 0, mod_rows = 0;
  for (int i = 0; i < (int)t.keys.size(); ++i) {
    // exact-size heap buffers: a write past namelen is an AddressSanitizer report
    const size_t len = t.keys[i].name.size();
    char* full = (char*)malloc(len + 1);
    int64_t shape[2] = {-7, -7};
    int32_t ndim = 0;
    CHECK(vckeys::describe(t, i, full, (int)len + 1, shape, &ndim, err, sizeof(err)) == VC_OK);
    CHECK(t.keys[i].name == full && seen.insert(full).second && vckeys::find(t, full) == i);
    CHECK(ndim == t.keys[i].ndim && shape[0] == t.keys[i].shape[0]);
    free(full);
    // a truncated namelen: namelen - 1 characters and a terminator, never more
    const int cut = len > 9 ? 9 : 1;
    char* part = (char*)malloc(cut);
    memset(part, 'x', cut);
    CHECK(vckeys::describe(t, i, part, cut, shape, &ndim, err, sizeof(err)) == VC_OK);
    CHECK(strlen(part) == (size_t)cut - 1 && !strncmp(part, t.keys[i].name.c_str(), cut - 1));
    free(part);
    // the shape parser: the key's own shape passes, a rank dimension takes 0 .. MAX_RANK, anything else names the key
    int64_t own[2] = {t.keys[i].shape[0] < 0 ? 16 : t.keys[i].shape[0], t.keys[i].shape[1] < 0 ? 16 : t.keys[i].shape[1]};
    CHECK(vckeys::check_shape(t.keys[i], own, t.keys[i].ndim, err, sizeof(err)) == VC_OK);
    int64_t off[2] = {own[0] + 1, own[1]};
    const bool rank0 = t.keys[i].shape[0] < 0;
    CHECK((vckeys::check_shape(t.keys[i], off, t.keys[i].ndim, err, sizeof(err)) == VC_OK) == rank0);
    if (!rank0) CHECK(strstr(err, t.keys[i].name.c_str()) != nullptr);
    CHECK(vckeys::check_shape(t.keys[i], own, 3 - t.keys[i].ndim, err, sizeof(err)) == VC_ERR_ARG && strstr(err, t.keys[i].name.c_str()));
    CHECK(vckeys::check_shape(t.keys[i], nullptr, t.keys[i].ndim, err, sizeof(err)) == VC_ERR_ARG);
    if (t.keys[i].shape[0] < 0 || (t.keys[i].ndim == 2 && t.keys[i].shape[1] < 0)) {
      int64_t r[2] = {own[0], own[1]};
      int64_t& rank = t.keys[i].shape[0] < 0 ? r[0] : r[1];
      rank = 0;                  CHECK(vckeys::check_shape(t.keys[i], r, 2, err, sizeof(err)) == VC_OK);
      rank = vckeys::MAX_RANK;   CHECK(vckeys::check_shape(t.keys[i], r, 2, err, sizeof(err)) == VC_OK);
      rank = vckeys::MAX_RANK + 1; CHECK(vckeys::check_shape(t.keys[i], r, 2, err, sizeof(err)) == VC_ERR_ARG);
      rank = -1;                 CHECK(vckeys::check_shape(t.keys[i], r, 2, err, sizeof(err)) == VC_ERR_ARG);
    }
  }
  // an index out of range, either side, and null / empty buffers
  char name[8];
  int64_t shape[2];
  int32_t ndim;
  CHECK(vckeys::describe(t, (int)t.keys.size(), name, sizeof(name), shape, &ndim, err, sizeof(err)) == VC_ERR_ARG && strstr(err, "index"));
  CHECK(vckeys::describe(t, -1, name, sizeof(name), shape, &ndim, err, sizeof(err)) == VC_ERR_ARG);
  CHECK(vckeys::describe(t, 1 << 30, name, sizeof(name), shape, &ndim, err, sizeof(err)) == VC_ERR_ARG);
  CHECK(vckeys::describe(t, 0, name, 0, shape, &ndim, err, sizeof(err)) == VC_ERR_ARG);
  CHECK(vckeys::describe(t, 0, nullptr, 8, shape, &ndim, err, sizeof(err)) == VC_ERR_ARG);
  // long and foreign keys
  const std::string lng(4096, 'k');
  CHECK(vckeys::find(t, lng.c_str()) == -1 && vckeys::find(t, "") == -1 && vckeys::find(t, nullptr) == -1);
  CHECK(vckeys::find(t, "img_in") == -1 && vckeys::find(t, "img_in.weight") == 0 && vckeys::find(t, "img_in.weight ") == -1);
  CHECK(vckeys::find(t, ("double_blocks." + std::to_string(cfg.depth) + ".img_attn.qkv.weight").c_str()) == -1);
  // every Linear owns five consecutive keys; the modulation Linears tile the stacked matrix in order; the arena formula
  for (const vckeys::Linear& l : t.linears) {
    CHECK(t.keys[l.key0 + vckeys::WEIGHT].name == l.name + ".weight" && t.keys[l.key0 + vckeys::LORA_B_BIAS].name == l.name + ".lora_B.bias");
    CHECK(l.qkv == (l.out >= 3 * D && (l.name.find(".qkv") != std::string::npos || l.name.find(".linear1") != std::string::npos)));
    if (l.mod_off >= 0) { CHECK(l.in == D && l.mod_off >= 0 && l.mod_off + l.out <= t.n_mod); mod_rows += l.out; }
    else bytes += c256(2 * (int64_t)l.out * l.in) + c256(2 * (int64_t)l.out);
  }
  CHECK(mod_rows == t.n_mod);
  bytes += c256(2 * t.n_mod * D) + c256(2 * t.n_mod) + 256 * (int64_t)scales + c256(4 * (int64_t)scales);
  CHECK(vckeys::arena_bytes(t, D) == bytes);
}

int main() {
  const VcFluxConfig tiny = {384, 64, 64, 128, 256, 2, 2, 2, 1024, 1, {16, 56, 56}, 10000};
  const VcFluxConfig full = {384, 64, 768, 4096, 3072, 24, 19, 38, 12288, 1, {16, 56, 56}, 10000};
  VcFluxConfig bare = tiny;          // no guidance embedder, no blocks at all
  bare.guidance_embed = 0; bare.depth = 0; bare.depth_single_blocks = 0;
  VcFluxConfig deep = tiny;          // three-digit block indices
  deep.depth = 101; deep.depth_single_blocks = 120;
  check(tiny); check(full); check(bare); check(deep);
  printf("flux_keys ok\n");
  return 0;
}
