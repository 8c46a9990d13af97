// flux_keys.h: the key table of a FLUX + LoRA checkpoint.  Host code only (no HIP header, no device): the order is that of
// FluxLoraWrapper(...).state_dict() - modules in registration order (models/model.py:43-73, modules/layers.py:87-117, 148-156,
// 199-230, 248-253), a Linear's own weight and bias in front of its lora_A.weight, lora_B.weight, lora_B.bias (modules/lora.py:66-67).
#include "flux_keys.h"
#include <stdio.h>
#include <string.h>

namespace vckeys {

namespace {

struct Builder {
  Table& t;
  int D;
  void linear(const std::string& name, int out, int in, bool qkv = false, int64_t mod_off = -1) {
    Linear l;
    l.name = name; l.out = out; l.in = in; l.qkv = qkv; l.mod_off = mod_off;
    l.key0 = (int)t.keys.size();
    const int owner = (int)t.linears.size();
    t.linears.push_back(l);
    key(name + ".weight", WEIGHT, owner, out, in, 2);
    key(name + ".bias", BIAS, owner, out, 0, 1);
    key(name + ".lora_A.weight", LORA_A, owner, -1, in, 2);
    key(name + ".lora_B.weight", LORA_B, owner, out, -1, 2);
    key(name + ".lora_B.bias", LORA_B_BIAS, owner, out, 0, 1);
  }
  void scale(const std::string& name) {
    t.scales.push_back(name);
    key(name, SCALE, (int)t.scales.size() - 1, 128, 0, 1);
  }
  void key(const std::string& name, Kind kind, int owner, int64_t s0, int64_t s1, int ndim) {
    Key k;
    k.name = name; k.kind = kind; k.owner = owner; k.shape[0] = s0; k.shape[1] = s1; k.ndim = ndim;
    t.index[name] = (int)t.keys.size();
    t.keys.push_back(k);
  }
  void embedder(const std::string& name, int in) {
    linear(name + ".in_layer", D, in);
    linear(name + ".out_layer", D, D);
  }
  void attn(const std::string& name) {
    linear(name + ".qkv", 3 * D, D, true);
    scale(name + ".norm.query_norm.scale");
    scale(name + ".norm.key_norm.scale");
    linear(name + ".proj", D, D);
  }
};

inline int64_t ceil256(int64_t v) { return (v + 255) & ~(int64_t)255; }

}  // namespace

Table build(const VcFluxConfig& c) {
  Table t;
  const int D = c.hidden_size, mlp = c.mlp_hidden;
  Builder b{t, D};
  // the stacking order of the "modulation" matrix (vc_flux_mod_offset): double blocks (img, txt), single blocks, the last layer
  const int64_t single0 = (int64_t)c.depth * 12 * D, final0 = single0 + (int64_t)c.depth_single_blocks * 3 * D;
  t.n_mod = final0 + 2 * D;
  b.linear("img_in", D, c.in_channels);
  b.embedder("time_in", 256);
  b.embedder("vector_in", c.vec_in_dim);
  if (c.guidance_embed) b.embedder("guidance_in", 256);
  b.linear("txt_in", D, c.context_in_dim);
  for (int i = 0; i < c.depth; ++i) {
    const std::string pf = "double_blocks." + std::to_string(i) + ".";
    const char* st[2] = {"img", "txt"};
    for (int k = 0; k < 2; ++k) {
      b.linear(pf + st[k] + "_mod.lin", 6 * D, D, false, ((int64_t)i * 2 + k) * 6 * D);
      b.attn(pf + st[k] + "_attn");
      b.linear(pf + st[k] + "_mlp.0", mlp, D);
      b.linear(pf + st[k] + "_mlp.2", D, mlp);
    }
  }
  for (int i = 0; i < c.depth_single_blocks; ++i) {
    const std::string pf = "single_blocks." + std::to_string(i) + ".";
    b.linear(pf + "linear1", 3 * D + mlp, D, true);
    b.linear(pf + "linear2", D, D + mlp);
    b.scale(pf + "norm.query_norm.scale");
    b.scale(pf + "norm.key_norm.scale");
    b.linear(pf + "modulation.lin", 3 * D, D, false, single0 + (int64_t)i * 3 * D);
  }
  b.linear("final_layer.linear", c.out_channels, D);
  b.linear("final_layer.adaLN_modulation.1", 2 * D, D, false, final0);
  return t;
}

int find(const Table& t, const char* key) {
  if (!key) return -1;
  auto it = t.index.find(key);
  return it == t.index.end() ? -1 : it->second;
}

int describe(const Table& t, int index, char* name, int namelen, int64_t* shape, int32_t* ndim, char* err, int errlen) {
  if (index < 0 || index >= (int)t.keys.size()) {
    snprintf(err, errlen, "flux_load_key: index = %d, the model has %d keys", index, (int)t.keys.size());
    return VC_ERR_ARG;
  }
  if (!name || namelen <= 0 || !shape || !ndim) {
    snprintf(err, errlen, "flux_load_key: null name / shape / ndim or namelen = %d", namelen);
    return VC_ERR_ARG;
  }
  const Key& k = t.keys[index];
  const size_t n = k.name.size() < (size_t)namelen - 1 ? k.name.size() : (size_t)namelen - 1;
  memcpy(name, k.name.data(), n);
  name[n] = 0;
  shape[0] = k.shape[0];
  shape[1] = k.ndim > 1 ? k.shape[1] : 0;
  *ndim = k.ndim;
  return VC_OK;
}

int check_shape(const Key& k, const int64_t* shape, int ndim, char* err, int errlen) {
  bool ok = shape && ndim == k.ndim;
  for (int d = 0; ok && d < k.ndim; ++d) ok = k.shape[d] < 0 ? shape[d] >= 0 && shape[d] <= MAX_RANK : shape[d] == k.shape[d];
  if (ok) return VC_OK;
  char want[64], got[64] = "null";
  auto dim = [](char* o, size_t n, int64_t v) { return v < 0 ? snprintf(o, n, "rank") : snprintf(o, n, "%lld", (long long)v); };
  int w = snprintf(want, sizeof(want), "[");
  for (int d = 0; d < k.ndim; ++d) { if (d) w += snprintf(want + w, sizeof(want) - w, ", "); w += dim(want + w, sizeof(want) - w, k.shape[d]); }
  snprintf(want + w, sizeof(want) - w, "]");
  if (shape) {
    int g = snprintf(got, sizeof(got), "[");
    for (int d = 0; d < ndim && d < 2; ++d) g += snprintf(got + g, sizeof(got) - g, d ? ", %lld" : "%lld", (long long)shape[d]);
    snprintf(got + g, sizeof(got) - g, ndim > 2 ? ", ...]" : "]");
  }
  snprintf(err, errlen, "flux_load_tensor: shape = %s of '%s' (%d dims), expected %s (rank: 0 .. %d)", got, k.name.c_str(), ndim, want, MAX_RANK);
  return VC_ERR_ARG;
}

int64_t arena_bytes(const Table& t, int hidden) {
  int64_t n = 0;
  for (const Linear& l : t.linears)
    if (l.mod_off < 0) n += ceil256(2 * (int64_t)l.out * l.in) + ceil256(2 * (int64_t)l.out);
  n += ceil256(2 * t.n_mod * hidden) + ceil256(2 * t.n_mod);
  n += 256 * (int64_t)t.scales.size() + ceil256(4 * (int64_t)t.scales.size());
  return n;
}

}  // namespace vckeys
