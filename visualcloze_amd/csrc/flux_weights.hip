// What is bound to a Flux handle (flux_state.h): the weights and LoRA pairs by name (vc_flux_bind_weight / _bind_lora), their
// resolution into the per-block tables the launch plan reads (resolve, at vc_flux_prepare), and a checkpoint as stored -> the bound set
// (vc_flux_load_*).  Host code only; the one thing it launches is the merge of vc_flux_load_finish.
#include "flux_state.h"

namespace vcflux {
namespace {

int find(Flux& f, const std::string& name, Lin& out, int N, int K, bool need_bias, Err e) {
  auto it = f.bound.find(name);
  if (it == f.bound.end()) FAIL(VC_ERR_STATE, "flux: weight '%s' is not bound", name.c_str());
  out = it->second;
  if (out.N != N || out.K != K) FAIL(VC_ERR_ARG, "flux: weight '%s' is [%d, %d], expected [%d, %d]", name.c_str(), out.N, out.K, N, K);
  if (need_bias && !out.b) FAIL(VC_ERR_ARG, "flux: weight '%s' needs a bias", name.c_str());
  return VC_OK;
}
int find_scale(Flux& f, const std::string& name, const void*& out, Err e) {
  auto it = f.bound.find(name);
  if (it == f.bound.end()) FAIL(VC_ERR_STATE, "flux: scale '%s' is not bound", name.c_str());
  if (it->second.N * it->second.K != 128) FAIL(VC_ERR_ARG, "flux: scale '%s' must hold 128 values", name.c_str());
  out = it->second.w;
  return VC_OK;
}

void layout_modulation(Flux& f) {
  int64_t o = 0;
  for (int i = 0; i < f.cfg.depth; ++i) {
    f.mod_off["double_blocks." + std::to_string(i) + ".img_mod.lin"] = o; o += 6 * f.D;
    f.mod_off["double_blocks." + std::to_string(i) + ".txt_mod.lin"] = o; o += 6 * f.D;
  }
  for (int i = 0; i < f.cfg.depth_single_blocks; ++i) { f.mod_off["single_blocks." + std::to_string(i) + ".modulation.lin"] = o; o += 3 * f.D; }
  f.mod_off["final_layer.adaLN_modulation.1"] = o; o += 2 * f.D;
  f.n_mod = o;
}

// max |scale| of a bound QK-norm scale vector (128 bf16 on the device): read back ONCE, when the weights are resolved
int scale_absmax(const void* dev, double& out, Err e) {
  uint16_t h[128];
  HIP(hipMemcpy(h, dev, sizeof(h), hipMemcpyDeviceToHost), "hipMemcpy (QK-norm scale)");
  out = vcrules::scale_absmax(h);
  return VC_OK;
}

// the pair bound for module `name` belongs to the Linear `l`, whose rows are [row0, row0 + l.N) of that module's
int attach_lora(Flux& f, const std::string& name, const Lin& l, int row0, Err e) {
  auto it = f.lora.find(name);
  if (it == f.lora.end()) return VC_OK;
  Lora lo = it->second;
  if (lo.in != l.K || row0 + l.N > lo.out)
    FAIL(VC_ERR_ARG, "flux: LoRA pair of '%s' is [%d, r] x [r, %d], its Linear takes %d inputs", name.c_str(), lo.out, lo.in, l.K);
  lo.b = (const bf16_t*)lo.b + (int64_t)row0 * lo.ldb;
  if (lo.bb) lo.bb = (const bf16_t*)lo.bb + row0;
  lo.out = l.N;
  f.lora_of[l.w] = lo;
  return VC_OK;
}

}  // namespace

int resolve(Flux& f, char* err, int errlen) {
  Err e{err, errlen};
  if (f.resolved) return VC_OK;
  const int D = f.D, mlp = f.mlp;
  f.lora_of.clear();
  f.mods.clear();
  TRY(find(f, "img_in", f.img_in, D, f.cfg.in_channels, false, e));
  TRY(find(f, "txt_in", f.txt_in, D, f.cfg.context_in_dim, false, e));
  TRY(find(f, "time_in.in_layer", f.time_in[0], D, 256, false, e));
  TRY(find(f, "time_in.out_layer", f.time_in[1], D, D, false, e));
  TRY(find(f, "vector_in.in_layer", f.vector_in[0], D, f.cfg.vec_in_dim, false, e));
  TRY(find(f, "vector_in.out_layer", f.vector_in[1], D, D, false, e));
  if (f.cfg.guidance_embed) {
    TRY(find(f, "guidance_in.in_layer", f.guidance_in[0], D, 256, false, e));
    TRY(find(f, "guidance_in.out_layer", f.guidance_in[1], D, D, false, e));
  }
  TRY(find(f, "final_layer.linear", f.final_lin, f.cfg.out_channels, D, false, e));
  TRY(find(f, "modulation", f.modulation, (int)f.n_mod, D, false, e));
  f.dbl.assign(f.cfg.depth, DoubleW{});
  for (int i = 0; i < f.cfg.depth; ++i) {
    const std::string pf = "double_blocks." + std::to_string(i) + ".";
    const char* st[2] = {"img", "txt"};
    for (int k = 0; k < 2; ++k) {
      const std::string a = pf + st[k] + "_attn.", m = pf + st[k] + "_mlp.";
      TRY(find(f, a + "qkv", f.dbl[i].qkv[k], 3 * D, D, false, e));
      TRY(find(f, a + "proj", f.dbl[i].proj[k], D, D, false, e));
      TRY(find(f, m + "0", f.dbl[i].mlp0[k], mlp, D, false, e));
      TRY(find(f, m + "2", f.dbl[i].mlp2[k], D, mlp, false, e));
      TRY(find_scale(f, a + "norm.query_norm.scale", f.dbl[i].qs[k], e));
      TRY(find_scale(f, a + "norm.key_norm.scale", f.dbl[i].ks[k], e));
      f.dbl[i].mod[k] = f.mod_off[pf + st[k] + "_mod.lin"];
    }
    double q[2], k2[2];
    for (int k = 0; k < 2; ++k) { TRY(scale_absmax(f.dbl[i].qs[k], q[k], e)); TRY(scale_absmax(f.dbl[i].ks[k], k2[k], e)); }
    f.dbl[i].bound = vcrules::logit_bound_of(q[0] > q[1] ? q[0] : q[1], k2[0] > k2[1] ? k2[0] : k2[1]);
  }
  f.sgl.assign(f.cfg.depth_single_blocks, SingleW{});
  for (int i = 0; i < f.cfg.depth_single_blocks; ++i) {
    const std::string pf = "single_blocks." + std::to_string(i) + ".";
    Lin l1;
    TRY(find(f, pf + "linear1", l1, 3 * D + mlp, D, false, e));
    SingleW& w = f.sgl[i];
    w.qkv = l1; w.qkv.N = 3 * D;                                  // linear1's rows [0, 3D) -> qkv, the rest -> mlp (layers.py:236)
    w.mlp = l1; w.mlp.N = mlp;
    w.mlp.w = (const bf16_t*)l1.w + (int64_t)3 * D * l1.ldw;
    w.mlp.b = l1.b ? (const void*)((const bf16_t*)l1.b + 3 * D) : nullptr;
    TRY(find(f, pf + "linear2", w.lin2, D, D + mlp, false, e));
    TRY(find_scale(f, pf + "norm.query_norm.scale", w.qs, e));
    TRY(find_scale(f, pf + "norm.key_norm.scale", w.ks, e));
    w.mod = f.mod_off[pf + "modulation.lin"];
    double q, k;
    TRY(scale_absmax(w.qs, q, e)); TRY(scale_absmax(w.ks, k, e));
    w.bound = vcrules::logit_bound_of(q, k);
  }
  f.final_mod = f.mod_off["final_layer.adaLN_modulation.1"];
  {  // the LoRA pairs (read in lora_mode 1 only)
    const char* plain[] = {"img_in", "txt_in", "final_layer.linear"};
    const Lin* plain_l[] = {&f.img_in, &f.txt_in, &f.final_lin};
    for (int i = 0; i < 3; ++i) TRY(attach_lora(f, plain[i], *plain_l[i], 0, e));
    const char* emb[] = {"time_in", "vector_in", "guidance_in"};
    Lin* emb_l[] = {f.time_in, f.vector_in, f.guidance_in};
    for (int i = 0; i < (f.cfg.guidance_embed ? 3 : 2); ++i) {
      TRY(attach_lora(f, std::string(emb[i]) + ".in_layer", emb_l[i][0], 0, e));
      TRY(attach_lora(f, std::string(emb[i]) + ".out_layer", emb_l[i][1], 0, e));
    }
    for (int i = 0; i < f.cfg.depth; ++i) {
      const std::string pf = "double_blocks." + std::to_string(i) + ".";
      const char* st[2] = {"img", "txt"};
      for (int k = 0; k < 2; ++k) {
        TRY(attach_lora(f, pf + st[k] + "_attn.qkv", f.dbl[i].qkv[k], 0, e));
        TRY(attach_lora(f, pf + st[k] + "_attn.proj", f.dbl[i].proj[k], 0, e));
        TRY(attach_lora(f, pf + st[k] + "_mlp.0", f.dbl[i].mlp0[k], 0, e));
        TRY(attach_lora(f, pf + st[k] + "_mlp.2", f.dbl[i].mlp2[k], 0, e));
      }
    }
    for (int i = 0; i < f.cfg.depth_single_blocks; ++i) {
      const std::string pf = "single_blocks." + std::to_string(i) + ".";
      TRY(attach_lora(f, pf + "linear1", f.sgl[i].qkv, 0, e));          // linear1's two row ranges share lora_A
      TRY(attach_lora(f, pf + "linear1", f.sgl[i].mlp, 3 * D, e));
      TRY(attach_lora(f, pf + "linear2", f.sgl[i].lin2, 0, e));
    }
    // every modulation Linear as the rows of the stacked matrix it owns, in stacking order
    std::vector<std::pair<int64_t, std::string>> order;
    for (const auto& kv : f.mod_off) order.push_back({kv.second, kv.first});
    std::sort(order.begin(), order.end());
    for (size_t i = 0; i < order.size(); ++i) {
      const int64_t off = order[i].first, end = i + 1 < order.size() ? order[i + 1].first : f.n_mod;
      Lin l = f.modulation;
      l.N = (int)(end - off);
      l.w = (const bf16_t*)f.modulation.w + off * f.modulation.ldw;
      l.b = f.modulation.b ? (const void*)((const bf16_t*)f.modulation.b + off) : nullptr;
      TRY(attach_lora(f, order[i].second, l, 0, e));
      f.mods.push_back({l, off});
    }
  }
  f.resolved = true;
  return VC_OK;
}

}  // namespace vcflux
using namespace vcflux;

int vc_flux_create_impl(const VcFluxConfig* cfg, void** handle, char* err, int errlen) {
  Err e{err, errlen};
  if (!cfg || !handle) FAIL(VC_ERR_ARG, "flux_create: null argument");
  if (cfg->hidden_size <= 0 || cfg->num_heads <= 0 || cfg->hidden_size != cfg->num_heads * 128)
    FAIL(VC_ERR_ARG, "flux_create: hidden_size must be num_heads * 128 (the gfx950 attention kernels are specialised for head_dim 128)");
  if (cfg->axes_dim[0] + cfg->axes_dim[1] + cfg->axes_dim[2] != 128 || (cfg->axes_dim[0] | cfg->axes_dim[1] | cfg->axes_dim[2]) & 1)
    FAIL(VC_ERR_ARG, "flux_create: axes_dim must be even and sum to 128");
  if (cfg->in_channels <= cfg->out_channels || cfg->out_channels <= 0 || cfg->depth < 0 || cfg->depth_single_blocks < 0 || cfg->mlp_hidden <= 0)
    FAIL(VC_ERR_ARG, "flux_create: bad channel / depth configuration");
  Flux* f = new Flux();
  f->cfg = *cfg;
  f->D = cfg->hidden_size; f->H = cfg->num_heads; f->mlp = cfg->mlp_hidden;
  layout_modulation(*f);
  f->keys = vckeys::build(*cfg);
  f->taps.assign((size_t)vcmon::tap_count(cfg->depth, cfg->depth_single_blocks), nullptr);
  // without a ROCm device the handle still answers its host-only calls (vc_flux_mod_offset, vc_flux_load_key / _tensor / _bytes,
  // vc_flux_bound); whatever touches the device then fails with the runtime's own error
  int dev = 0;
  hipDeviceProp_t p;
  if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&p, dev) == hipSuccess) {
    f->n_cu = p.multiProcessorCount;
    if (hipEventCreateWithFlags(&f->staged, hipEventDisableTiming) != hipSuccess) { delete f; FAIL(VC_ERR_HIP, "flux_create: hipEventCreate failed"); }
  }
  *handle = f;
  return VC_OK;
}

int vc_flux_bind_weight_impl(void* handle, const char* name, const void* w, const void* bias, int32_t rows, int32_t cols, int64_t ldw,
                             char* err, int errlen) {
  HANDLE(Flux, f, "flux");
  if (!name || !w || rows <= 0 || cols <= 0 || ldw < cols) FAIL(VC_ERR_ARG, "flux_bind_weight: bad arguments for '%s'", name ? name : "?");
  // the optional split-K scratch decides whether 100 MB are carved into EVERY workspace: binding it for the first time after a
  // workspace has been sized would silently change the carve-up of buffers the caller already holds (advisor r05)
  if (!strcmp(name, "splitk_ws") && f.ws_sized && f.bound.find("splitk_ws") == f.bound.end())
    FAIL(VC_ERR_STATE, "flux_bind_weight: bind 'splitk_ws' BEFORE the first vc_flux_workspace_bytes / vc_flux_prepare (it changes the size and "
                       "layout of every workspace)");
  Lin l;
  l.w = w; l.b = bias; l.N = rows; l.K = cols; l.ldw = ldw;
  f.bound[name] = l;
  f.resolved = false;
  f.prepared = false;   // the resolved per-block tables are rebuilt by the next vc_flux_prepare
  drop_graph(f);        // a captured step holds the old pointers
  return VC_OK;
}

// ---------------------------------------------------------------- a checkpoint as stored -> the bound set (vc_flux_load_*)
int vc_flux_load_key_impl(void* handle, int32_t index, char* name, int32_t namelen, int64_t* shape, int32_t* ndim, char* err, int errlen) {
  HANDLE(Flux, f, "flux");
  return vckeys::describe(f.keys, index, name, namelen, shape, ndim, err, errlen);
}

int vc_flux_load_tensor_impl(void* handle, const char* key, const void* ptr, int32_t is_f32, const int64_t* shape, int32_t ndim, char* err,
                             int errlen) {
  HANDLE(Flux, f, "flux");
  const int idx = vckeys::find(f.keys, key);
  if (idx < 0) FAIL(VC_ERR_ARG, "flux_load_tensor: key = '%s' is no state_dict key of this model (vc_flux_load_key lists them)", key ? key : "(null)");
  if (!ptr) { f.loaded.erase(idx); return VC_OK; }
  const vckeys::Key& k = f.keys.keys[idx];
  TRY(vckeys::check_shape(k, shape, ndim, err, errlen));
  const bool factor = k.kind == vckeys::LORA_A || k.kind == vckeys::LORA_B || k.kind == vckeys::LORA_B_BIAS;
  if (factor && is_f32)
    FAIL(VC_ERR_ARG, "flux_load_tensor: is_f32 = 1 for '%s': LoRA factors are merged on the bf16 matrix cores and must be stored as bf16", key);
  if (k.kind == vckeys::LORA_A || k.kind == vckeys::LORA_B) {      // one rank per Linear
    const int key0 = f.keys.linears[k.owner].key0;
    auto other = f.loaded.find(key0 + (k.kind == vckeys::LORA_A ? vckeys::LORA_B : vckeys::LORA_A));
    const int64_t rank = shape[k.kind == vckeys::LORA_A ? 0 : 1];
    if (other != f.loaded.end() && other->second.shape[k.kind == vckeys::LORA_A ? 1 : 0] != rank)
      FAIL(VC_ERR_ARG, "flux_load_tensor: rank = %lld of '%s' differs from the rank %lld of the Linear's other factor", (long long)rank, key,
           (long long)other->second.shape[k.kind == vckeys::LORA_A ? 1 : 0]);
  }
  f.loaded[idx] = Flux::Loaded{ptr, is_f32 != 0, {shape[0], ndim > 1 ? shape[1] : 0}};
  return VC_OK;
}

int64_t vc_flux_load_bytes_impl(void* handle) { return handle ? vckeys::arena_bytes(((Flux*)handle)->keys, ((Flux*)handle)->D) : -1; }

int vc_flux_load_finish_impl(void* handle, float lora_scale, void* arena, int64_t arena_bytes, hipStream_t s, char* err, int errlen) {
  HANDLE(Flux, f, "flux");
  const vckeys::Table& t = f.keys;
  // ---- every check before the device is touched
  if (f.opt.lora_mode)
    FAIL(VC_ERR_ARG, "flux_load_finish: option lora_mode = 1 runs un-merged weights (vc_flux_bind_weight + vc_flux_bind_lora); this call merges");
  if (f.in_flight) FAIL(VC_ERR_STATE, "flux_load_finish: the weights cannot change between vc_flux_sample_begin and vc_flux_sample_end");
  const int64_t need = vckeys::arena_bytes(t, f.D);
  if (!aligned256(arena)) FAIL(VC_ERR_ARG, "flux_load_finish: arena must be a 256-byte aligned device pointer");
  if (arena_bytes < need)
    FAIL(VC_ERR_ARG, "flux_load_finish: arena_bytes = %lld, the prepared set takes %lld (vc_flux_load_bytes)", (long long)arena_bytes, (long long)need);
  auto have = [&](int idx) -> const Flux::Loaded* {
    auto it = f.loaded.find(idx);
    return it == f.loaded.end() ? nullptr : &it->second;
  };
  for (size_t i = 0; i < t.keys.size(); ++i)
    if ((t.keys[i].kind == vckeys::WEIGHT || t.keys[i].kind == vckeys::SCALE) && !have((int)i))
      FAIL(VC_ERR_STATE, "flux_load_finish: '%s' was never recorded (vc_flux_load_tensor)", t.keys[i].name.c_str());
  for (const vckeys::Linear& l : t.linears)
    if (!have(l.key0 + vckeys::LORA_A) != !have(l.key0 + vckeys::LORA_B))
      FAIL(VC_ERR_STATE, "flux_load_finish: '%s' was recorded without the Linear's other factor",
           t.keys[l.key0 + (have(l.key0 + vckeys::LORA_A) ? vckeys::LORA_A : vckeys::LORA_B)].name.c_str());
  // ---- the arena: the formula of vc_flux_load_bytes, in its order
  Carver c{(char*)arena};
  std::vector<std::pair<std::string, Lin>> bind;
  std::vector<bf16_t*> wout(t.linears.size()), bout(t.linears.size());
  for (size_t i = 0; i < t.linears.size(); ++i) {
    const vckeys::Linear& l = t.linears[i];
    if (l.mod_off >= 0) continue;
    wout[i] = c.take<bf16_t>((int64_t)l.out * l.in);
    bout[i] = c.take<bf16_t>(l.out);
  }
  bf16_t* mod_w = c.take<bf16_t>(t.n_mod * f.D);
  bf16_t* mod_b = c.take<bf16_t>(t.n_mod);
  const int n_scales = (int)t.scales.size();
  bf16_t* scales = c.take<bf16_t>((int64_t)128 * n_scales);       // 256 bytes each
  float* amax = c.take<float>(n_scales);
  // ---- one merge launch per Linear (a modulation Linear without any bias leaves zeros in the stacked bias, as Flux.prepare does)
  HIP(hipMemsetAsync(mod_b, 0, (size_t)t.n_mod * 2, s), "hipMemsetAsync");
  for (size_t i = 0; i < t.linears.size(); ++i) {
    const vckeys::Linear& l = t.linears[i];
    const Flux::Loaded *w = have(l.key0 + vckeys::WEIGHT), *b = have(l.key0 + vckeys::BIAS), *la = have(l.key0 + vckeys::LORA_A),
                       *lb = have(l.key0 + vckeys::LORA_B), *lbb = have(l.key0 + vckeys::LORA_B_BIAS);
    const int rank = la ? (int)la->shape[0] : 0;
    if (!rank) la = lb = lbb = nullptr;                            // no pair: a conversion / copy (lora_B.bias belongs to the pair)
    const bool mod = l.mod_off >= 0;
    bf16_t* out = mod ? mod_w + l.mod_off * f.D : wout[i];
    bf16_t* bias_out = !(b || lbb) ? nullptr : mod ? mod_b + l.mod_off : bout[i];
    TRY(vc_lora_merge_qkv_launch(w->p, w->f32, l.in, la ? la->p : nullptr, l.in, lb ? lb->p : nullptr, rank, lora_scale, out, mod ? f.D : l.in,
                                 b ? b->p : nullptr, b ? b->f32 : 0, lbb ? lbb->p : nullptr, bias_out, l.out, l.in, rank, l.qkv ? f.H : 0, s,
                                 err, errlen));
    if (!mod) { Lin x; x.w = out; x.b = bias_out; x.N = l.out; x.K = l.in; x.ldw = l.in; bind.push_back({l.name, x}); }
  }
  { Lin x; x.w = mod_w; x.b = mod_b; x.N = (int)t.n_mod; x.K = f.D; x.ldw = f.D; bind.push_back({"modulation", x}); }
  // ---- the scales: one launch (per VC_SCALE_VECTORS of them), one read of their maxima
  for (int i0 = 0; i0 < n_scales; i0 += VC_SCALE_VECTORS) {
    VcScaleVectors v;
    memset(&v, 0, sizeof(v));
    const int n = std::min(VC_SCALE_VECTORS, n_scales - i0);
    for (int i = 0; i < n; ++i) {
      const Flux::Loaded* sc = have(vckeys::find(t, t.scales[i0 + i].c_str()));
      v.src[i] = sc->p; v.f32[i] = (uint8_t)sc->f32;
    }
    TRY(vc_scale_cast_launch(v, n, scales + (int64_t)128 * i0, 128, amax + i0, s, err, errlen));
  }
  std::vector<float> mx(n_scales);
  HIP(hipMemcpyAsync(mx.data(), amax, sizeof(float) * n_scales, hipMemcpyDeviceToHost, s), "hipMemcpyAsync (QK-norm maxima)");
  HIP(hipStreamSynchronize(s), "hipStreamSynchronize");
  // the cap Flux.prepare / Flux.handle() hand over: the largest per-block bound, in thousandths, rounded up; 0 (no bounded softmax
  // anywhere) where a scale is NaN or the bound leaves the option's range
  const int milli = vcrules::logit_cap_milli(vcrules::logit_cap(mx.data(), n_scales, f.cfg.depth));
  // ---- bind, as vc_flux_bind_weight would
  for (auto& kv : bind) f.bound[kv.first] = kv.second;
  for (int i = 0; i < n_scales; ++i) {
    Lin x; x.w = scales + (int64_t)128 * i; x.b = nullptr; x.N = 1; x.K = 128; x.ldw = 128;
    f.bound[t.scales[i]] = x;
  }
  f.opt.qkv_heads = f.H; f.opt.fuse_knorm = 1; f.opt.logit_bound_milli = milli;
  f.resolved = false;
  f.prepared = false;
  drop_graph(f);
  return VC_OK;
}

int vc_flux_bound_impl(void* handle, const char* name, const void** w, const void** bias, int32_t* rows, int32_t* cols, int64_t* ldw, char* err,
                       int errlen) {
  HANDLE(Flux, f, "flux");
  if (!name) FAIL(VC_ERR_ARG, "flux_bound: null name");
  auto it = f.bound.find(name);
  if (it == f.bound.end()) FAIL(VC_ERR_STATE, "flux_bound: nothing is bound under '%s'", name);
  if (w) *w = it->second.w;
  if (bias) *bias = it->second.b;
  if (rows) *rows = it->second.N;
  if (cols) *cols = it->second.K;
  if (ldw) *ldw = it->second.ldw;
  return VC_OK;
}

int64_t vc_flux_mod_offset_impl(void* handle, const char* name) {
  if (!handle) return -1;
  Flux& f = *(Flux*)handle;
  if (!name) return f.n_mod;
  auto it = f.mod_off.find(name);
  return it == f.mod_off.end() ? -1 : it->second;
}

int vc_flux_bind_lora_impl(void* handle, const char* name, const void* lora_a, int64_t lda, const void* lora_b, int64_t ldb,
                           const void* lora_b_bias, int32_t out_features, int32_t in_features, int32_t rank, char* err, int errlen) {
  HANDLE(Flux, f, "flux");
  if (!name) FAIL(VC_ERR_ARG, "flux_bind_lora: null name");
  if (!lora_a && !lora_b) {           // unbind
    f.lora.erase(name);
  } else {
    if (!lora_a || !lora_b) FAIL(VC_ERR_ARG, "flux_bind_lora: lora_a and lora_b of '%s' must both be given", name);
    if (rank <= 0 || rank % 64)
      FAIL(VC_ERR_ARG, "flux_bind_lora: rank = %d of '%s' must be a positive multiple of 64, the GEMM's K granularity (zero-pad the factors)", rank, name);
    int out = 0, in = 0;              // what the Linear is: a module of the stacked modulation matrix, or a bound weight
    auto mo = f.mod_off.find(name);
    if (mo != f.mod_off.end()) {
      int64_t end = f.n_mod;
      for (const auto& kv : f.mod_off) if (kv.second > mo->second && kv.second < end) end = kv.second;
      out = (int)(end - mo->second); in = f.D;
    } else {
      auto it = f.bound.find(name);
      if (it == f.bound.end()) FAIL(VC_ERR_STATE, "flux_bind_lora: name = '%s' is no Linear bound by vc_flux_bind_weight (bind the weight first)", name);
      out = it->second.N; in = it->second.K;
    }
    if (out_features != out || in_features != in)
      FAIL(VC_ERR_ARG, "flux_bind_lora: out_features, in_features = %d, %d of '%s', its weight is [%d, %d]", out_features, in_features, name, out, in);
    if (lda < in || ldb < rank || lda % 8 || ldb % 8)
      FAIL(VC_ERR_ARG, "flux_bind_lora: lda = %lld, ldb = %lld of '%s' must be multiples of 8, at least in_features and rank", (long long)lda, (long long)ldb, name);
    Lora lo;
    lo.a = lora_a; lo.b = lora_b; lo.bb = lora_b_bias; lo.rank = rank; lo.out = out; lo.in = in; lo.lda = lda; lo.ldb = ldb;
    f.lora[name] = lo;
  }
  f.resolved = false;
  f.prepared = false;   // the widest rank sizes the workspace
  drop_graph(f);
  return VC_OK;
}

int vc_flux_set_lora_scale_impl(void* handle, float scale, char* err, int errlen) {
  HANDLE(Flux, f, "flux");
  if (!(scale - scale == 0.0f) || vcrules::bf16_round(scale) != scale)
    FAIL(VC_ERR_ARG, "flux_set_lora_scale: scale = %.9g is not a bf16 value; the un-merged mode applies it as a bf16 vector and would round it "
                     "(merge with vc_lora_merge, which applies any scale in f32)", scale);
  if (f.in_flight)      // the trajectory's modulation rows and its step-invariant projections ran with the old scale
    FAIL(VC_ERR_STATE, "flux_set_lora_scale: scale cannot change between vc_flux_sample_begin and vc_flux_sample_end");
  // host only.  The next vc_flux_prepare writes the value into the scale vector, which keeps its place in that workspace: a step
  // captured there replays with it.  Until then the prepared state is of the old scale and forward / sample_begin refuse it
  if (scale != f.lora_scale && f.prepared) f.scale_stale = true;
  f.lora_scale = scale;
  return VC_OK;
}
