// Text-encoder handle of include/vcloze_hip.h: T5EncoderModel (last_hidden_state) and CLIPTextModel (last_hidden_state, pooler_output),
// the two inputs `txt` / `y` of vc_flux_prepare (reference call site models/modules/conditioner.py:5-37), as launch plans over the
// kernels of this library.  Host code only: it ORDERS launches - the order visualcloze_amd/text.py spells in Python over the op-level
// ABI (the parity twin: same kernels, same problem structs, same order, same bits) - once per (workspace, L, stream) under stream
// capture.  What text.py does in torch between two launches is here
//   the relative-position-bias table (bucket ids, fancy index, permute)    vc_t5_position_bias, once per prepare / re-bind
//   CLIP's zero-padded ids, zeroed position rows and their sum             vc_clip_embed, one launch of the plan
//   CLIP's argmax over (ids == eos) and the advanced index                  vc_clip_pool, the plan's last launch (no host read-back)
//   the residual gate of ones                                               one 16-bit memset at prepare time
// Weights are bound BY POINTER (bf16, as state_dict() stores them): no copy, no allocation.
//
// Workspace (caller's device memory), bf16 unless noted, named like text.py's scratch pool; R = L (T5) or ceil64(L) (CLIP) rows:
//   IDS int32 [L]   the prompt in flight        OUT [R, D]   the final norm's output        POOL [D]   CLIP's pooler_output
//   X N [R, D]      residual stream, its norm   Q K V O [R, H dh]                           S [H R, R]  scores, then probabilities
//   VT [H dh, R]    V^T                         FA FB [R, d_ff]  the FF pair (g / u, f1 / f2)
//   ONES [D]        the gate of `x + h`         BIAS [H L, L]    T5's position bias
#include "common.h"
#include "vcloze_internal.h"
#include "engine_core.h"
#include <math.h>
#include <string.h>
#include <string>
#include <unordered_map>
#include <vector>

namespace {

// one state_dict entry
struct Tensor {
  std::string key;
  int ndim = 1;
  int64_t shape[2] = {0, 0};
  bool read = true;          // false: accepted and shape-checked, never read (T5's tied encoder.embed_tokens.weight)
  const bf16_t* p = nullptr;
};
struct Lin { int w = -1, b = -1; };
struct T5Layer { Lin q, k, v, o, wi0, wi1, wo; int ln0 = -1, ln1 = -1; };
struct ClipLayer { Lin q, k, v, o, fc1, fc2; Lin ln1, ln2; };

enum BufId { IDS, OUT, POOL, X, N, Q, K, V, S, VT, O, FA, FB, ONES, BIAS, NBUF };

struct Text {
  VcTextConfig cfg{};
  int D = 0, H = 0, dh = 0, F = 0;
  std::vector<Tensor> t;
  std::unordered_map<std::string, int> by_key;
  int emb = -1, pos = -1, rel = -1;
  Lin fin;
  std::vector<T5Layer> t5;
  std::vector<ClipLayer> clip;
  // prepared geometry + workspace carve-up
  bool prepared = false, bias_ready = false;
  int L = 0, R = 0;
  char* base = nullptr;
  char* ptr[NBUF] = {};
  // captured plans, most recently used first
  struct Key {
    char* base; int L; hipStream_t s;
    bool operator==(const Key& o) const { return base == o.base && L == o.L && s == o.s; }
  };
  PlanCache<Key, hipGraphExec_t, 8, DropExec> plans;
  std::vector<int> warmed;   // the L whose launches have run un-captured once on this handle (kernel attributes are set on a first launch)
};

// ---------------------------------------------------------------- the state dict of text.T5EncoderModel / text.CLIPTextModel, in order
int add(Text& v, const std::string& key, int64_t d0, int64_t d1 = 0, bool read = true) {
  Tensor t;
  t.key = key; t.ndim = d1 ? 2 : 1; t.shape[0] = d0; t.shape[1] = d1; t.read = read;
  v.t.push_back(t);
  v.by_key[key] = (int)v.t.size() - 1;
  return (int)v.t.size() - 1;
}
Lin add_lin(Text& v, const std::string& p, int64_t out, int64_t in, bool bias) {
  Lin l;
  l.w = add(v, p + ".weight", out, in);
  if (bias) l.b = add(v, p + ".bias", out);
  return l;
}
Lin add_norm(Text& v, const std::string& p, int64_t d, bool bias) {
  Lin l;
  l.w = add(v, p + ".weight", d);
  if (bias) l.b = add(v, p + ".bias", d);
  return l;
}
void build_tree(Text& v) {
  const VcTextConfig& c = v.cfg;
  char nm[128];
  if (c.kind == VC_TEXT_T5) {
    const int64_t inner = (int64_t)v.H * v.dh;
    v.emb = add(v, "shared.weight", c.vocab_size, v.D);
    add(v, "encoder.embed_tokens.weight", c.vocab_size, v.D, false);
    for (int i = 0; i < c.num_layers; ++i) {
      T5Layer l;
      snprintf(nm, sizeof(nm), "encoder.block.%d.layer.0.SelfAttention", i);
      const std::string a(nm);
      l.q = add_lin(v, a + ".q", inner, v.D, false);
      l.k = add_lin(v, a + ".k", inner, v.D, false);
      l.v = add_lin(v, a + ".v", inner, v.D, false);
      l.o = add_lin(v, a + ".o", v.D, inner, false);
      if (i == 0) v.rel = add(v, a + ".relative_attention_bias.weight", c.num_buckets, v.H);
      snprintf(nm, sizeof(nm), "encoder.block.%d.layer.0.layer_norm", i);
      l.ln0 = add_norm(v, nm, v.D, false).w;
      snprintf(nm, sizeof(nm), "encoder.block.%d.layer.1.DenseReluDense", i);
      const std::string f(nm);
      l.wi0 = add_lin(v, f + ".wi_0", v.F, v.D, false);
      l.wi1 = add_lin(v, f + ".wi_1", v.F, v.D, false);
      l.wo = add_lin(v, f + ".wo", v.D, v.F, false);
      snprintf(nm, sizeof(nm), "encoder.block.%d.layer.1.layer_norm", i);
      l.ln1 = add_norm(v, nm, v.D, false).w;
      v.t5.push_back(l);
    }
    v.fin = add_norm(v, "encoder.final_layer_norm", v.D, false);
  } else {
    v.emb = add(v, "text_model.embeddings.token_embedding.weight", c.vocab_size, v.D);
    v.pos = add(v, "text_model.embeddings.position_embedding.weight", c.max_positions, v.D);
    for (int i = 0; i < c.num_layers; ++i) {
      ClipLayer l;
      snprintf(nm, sizeof(nm), "text_model.encoder.layers.%d", i);
      const std::string p(nm);
      l.k = add_lin(v, p + ".self_attn.k_proj", v.D, v.D, true);
      l.v = add_lin(v, p + ".self_attn.v_proj", v.D, v.D, true);
      l.q = add_lin(v, p + ".self_attn.q_proj", v.D, v.D, true);
      l.o = add_lin(v, p + ".self_attn.out_proj", v.D, v.D, true);
      l.ln1 = add_norm(v, p + ".layer_norm1", v.D, true);
      l.fc1 = add_lin(v, p + ".mlp.fc1", v.F, v.D, true);
      l.fc2 = add_lin(v, p + ".mlp.fc2", v.D, v.F, true);
      l.ln2 = add_norm(v, p + ".layer_norm2", v.D, true);
      v.clip.push_back(l);
    }
    v.fin = add_norm(v, "text_model.final_layer_norm", v.D, true);
  }
}

// ---------------------------------------------------------------- the plan (text.py: _Exec, T5EncoderModel._run, CLIPTextModel._encode_one)
struct Run {
  Text& v; hipStream_t s; Err e;
  bf16_t* b(int id) const { return (bf16_t*)v.ptr[id]; }
  const bf16_t* w(int i) const { return i < 0 ? nullptr : v.t[i].p; }
};

// hip.make_problem(a, w, bias, out[, res, gate = ones, rows_per_batch = M]): contiguous operands
void problem(VcGemmProblem& p, const void* A, int64_t lda, const void* W, int64_t ldw, const void* bias, void* C, int64_t ldc, int M, int Nn, int Kk) {
  memset(&p, 0, sizeof(p));
  p.A = A; p.W = W; p.bias = bias; p.C = C;
  p.lda = lda; p.ldw = ldw; p.ldc = ldc;
  p.M = M; p.N = Nn; p.K = Kk; p.rows_per_batch = M;
}
// _Exec._linear: out = epi(a @ w^T + b), or out = res + (a @ w^T + b) through the gated-residual epilogue with a gate of ones
int linear(Run& r, const Lin& l, const bf16_t* a, int M, int Kk, bf16_t* out, int Nn, int epi, const bf16_t* res = nullptr) {
  VcGemmArgs g;
  memset(&g, 0, sizeof(g));
  g.nprob = 1;
  g.epi = res ? VC_EPI_GATE_RES : epi;
  problem(g.p[0], a, Kk, r.w(l.w), Kk, r.w(l.b), out, Nn, M, Nn, Kk);
  if (res) { g.p[0].res = res; g.p[0].ldres = Nn; g.p[0].gate = r.b(ONES); }
  return vc_gemm_launch(g, 0, r.s, r.e.buf, r.e.len);
}
// the grouped q / k / v projection of one layer: three problems, one launch
int qkv(Run& r, const Lin& q, const Lin& k, const Lin& v, int M, int Kk, int Nn) {
  VcGemmArgs g;
  memset(&g, 0, sizeof(g));
  g.nprob = 3;
  g.epi = VC_EPI_BIAS;
  problem(g.p[0], r.b(N), Kk, r.w(q.w), Kk, r.w(q.b), r.b(Q), Nn, M, Nn, Kk);
  problem(g.p[1], r.b(N), Kk, r.w(k.w), Kk, r.w(k.b), r.b(K), Nn, M, Nn, Kk);
  problem(g.p[2], r.b(N), Kk, r.w(v.w), Kk, r.w(v.b), r.b(V), Nn, M, Nn, Kk);
  return vc_gemm_launch(g, 0, r.s, r.e.buf, r.e.len);
}
// _Exec._heads_attention: S_h = q_h k_h^T for all heads in one batched launch, row softmax, V^T, O_h = P_h V_h in one more
int heads_attention(Run& r, int R, float scale, const bf16_t* bias, int causal_period) {
  const int H = r.v.H, dh = r.v.dh, inner = H * dh;
  VcGemmArgs g;
  memset(&g, 0, sizeof(g));
  g.nprob = 1; g.epi = VC_EPI_BIAS; g.batch = H;
  problem(g.p[0], r.b(Q), inner, r.b(K), inner, nullptr, r.b(S), R, R, R, dh);
  g.p[0].a_zstride = dh; g.p[0].w_zstride = dh; g.p[0].c_zstride = (int64_t)R * R;
  TRY(vc_gemm_launch(g, 0, r.s, r.e.buf, r.e.len));
  TRY(vc_softmax_rows_launch(r.b(S), R, H * R, R, scale, bias, bias ? R : 0, causal_period, r.s, r.e.buf, r.e.len));
  TRY(vc_transpose_launch(r.b(V), inner, r.b(VT), R, R, inner, r.s, r.e.buf, r.e.len));
  memset(&g, 0, sizeof(g));
  g.nprob = 1; g.epi = VC_EPI_BIAS; g.batch = H;
  problem(g.p[0], r.b(S), R, r.b(VT), R, nullptr, r.b(O), inner, R, dh, R);
  g.p[0].a_zstride = (int64_t)R * R; g.p[0].w_zstride = (int64_t)dh * R; g.p[0].c_zstride = dh;
  return vc_gemm_launch(g, 0, r.s, r.e.buf, r.e.len);
}

int t5_plan(Run& r) {
  Text& v = r.v;
  const int L = v.L, D = v.D, inner = v.H * v.dh, F = v.F;
  const float eps = v.cfg.eps;
  TRY(vc_embedding_launch((const int32_t*)v.ptr[IDS], r.w(v.emb), D, v.cfg.vocab_size, r.b(X), L, D, r.s, r.e.buf, r.e.len));
  for (const T5Layer& l : v.t5) {
    TRY(vc_rownorm_launch(r.b(X), r.w(l.ln0), nullptr, r.b(N), L, D, eps, 0, r.s, r.e.buf, r.e.len));
    TRY(qkv(r, l.q, l.k, l.v, L, D, inner));
    TRY(heads_attention(r, L, 1.0f, r.b(BIAS), 0));                       // T5 does not scale the scores
    TRY(linear(r, l.o, r.b(O), L, inner, r.b(X), D, VC_EPI_BIAS, r.b(X)));
    TRY(vc_rownorm_launch(r.b(X), r.w(l.ln1), nullptr, r.b(N), L, D, eps, 0, r.s, r.e.buf, r.e.len));
    TRY(linear(r, l.wi0, r.b(N), L, D, r.b(FA), F, VC_EPI_GELU));         // gelu_new = tanh GELU
    TRY(linear(r, l.wi1, r.b(N), L, D, r.b(FB), F, VC_EPI_BIAS));
    TRY(vc_ewise_launch(r.b(FA), r.b(FB), r.b(FA), (int64_t)L * F, 0, r.s, r.e.buf, r.e.len));
    TRY(linear(r, l.wo, r.b(FA), L, F, r.b(X), D, VC_EPI_BIAS, r.b(X)));
  }
  return vc_rownorm_launch(r.b(X), r.w(v.fin.w), nullptr, r.b(OUT), L, D, eps, 0, r.s, r.e.buf, r.e.len);
}

int clip_plan(Run& r) {
  Text& v = r.v;
  const int L = v.L, R = v.R, D = v.D, F = v.F;
  const float eps = v.cfg.eps;
  const int32_t* ids = (const int32_t*)v.ptr[IDS];
  TRY(vc_clip_embed_launch(ids, r.w(v.emb), D, v.cfg.vocab_size, r.w(v.pos), D, r.b(X), L, R, D, r.s, r.e.buf, r.e.len));
  for (const ClipLayer& l : v.clip) {
    TRY(vc_rownorm_launch(r.b(X), r.w(l.ln1.w), r.w(l.ln1.b), r.b(N), R, D, eps, 1, r.s, r.e.buf, r.e.len));
    TRY(qkv(r, l.q, l.k, l.v, R, D, D));
    TRY(heads_attention(r, R, (float)pow((double)v.dh, -0.5), nullptr, R));     // rows L..R-1 are padding: causal masking keeps them out of rows < L
    TRY(linear(r, l.o, r.b(O), R, D, r.b(X), D, VC_EPI_BIAS, r.b(X)));
    TRY(vc_rownorm_launch(r.b(X), r.w(l.ln2.w), r.w(l.ln2.b), r.b(N), R, D, eps, 1, r.s, r.e.buf, r.e.len));
    TRY(linear(r, l.fc1, r.b(N), R, D, r.b(FA), F, VC_EPI_BIAS));
    TRY(vc_ewise_launch(r.b(FA), nullptr, r.b(FB), (int64_t)R * F, 2, r.s, r.e.buf, r.e.len));
    TRY(linear(r, l.fc2, r.b(FB), R, F, r.b(X), D, VC_EPI_BIAS, r.b(X)));
  }
  TRY(vc_rownorm_launch(r.b(X), r.w(v.fin.w), r.w(v.fin.b), r.b(OUT), R, D, eps, 1, r.s, r.e.buf, r.e.len));
  return vc_clip_pool_launch(ids, r.b(OUT), D, L, D, v.cfg.eos_token_id, r.b(POOL), r.s, r.e.buf, r.e.len);
}

int check_len(const Text& v, int L, Err e, const char* what) {
  if (v.cfg.kind == VC_TEXT_T5) {
    if (L <= 0 || L % 64 || L > 16384) FAIL(VC_ERR_ARG, "%s: a T5 sequence length must be a positive multiple of 64 up to 16384, got %d", what, L);
  } else if (L <= 0 || L > v.cfg.max_positions) {
    FAIL(VC_ERR_ARG, "%s: a CLIP sequence length must be 1..max_positions = %d, got %d", what, v.cfg.max_positions, L);
  }
  return VC_OK;
}
// the carve-up of the workspace at sequence length L; returns the bytes it takes
int64_t carve(const Text& v, int L, char* base, char* ptr[NBUF]) {
  const bool t5 = v.cfg.kind == VC_TEXT_T5;
  const int64_t R = t5 ? L : (L + 63) / 64 * 64, D = v.D, inner = (int64_t)v.H * v.dh, F = v.F;
  int64_t bytes[NBUF] = {};
  bytes[IDS] = (int64_t)L * 4;
  bytes[OUT] = bytes[X] = bytes[N] = R * D * 2;
  bytes[POOL] = t5 ? 0 : D * 2;
  bytes[Q] = bytes[K] = bytes[V] = bytes[O] = bytes[VT] = R * inner * 2;
  bytes[S] = (int64_t)v.H * R * R * 2;
  bytes[FA] = bytes[FB] = R * F * 2;
  bytes[ONES] = D * 2;
  bytes[BIAS] = t5 ? bytes[S] : 0;
  Carver c{base};
  for (int i = 0; i < NBUF; ++i) ptr[i] = c.bytes(bytes[i]);
  return c.off;
}

int build_bias(Text& v, hipStream_t s, Err e) {
  const Tensor& t = v.t[v.rel];
  TRY(vc_t5_position_bias_launch(t.p, v.H, v.H, v.L, v.cfg.num_buckets, v.cfg.max_distance, v.ptr[BIAS], s, e.buf, e.len));
  v.bias_ready = true;
  return VC_OK;
}

}  // namespace

int vc_text_create_impl(const VcTextConfig* cfg, void** handle, char* err, int errlen) {
  Err e{err, errlen};
  if (!cfg || !handle) FAIL(VC_ERR_ARG, "text_create: null argument");
  const VcTextConfig& c = *cfg;
  if (c.kind != VC_TEXT_T5 && c.kind != VC_TEXT_CLIP) FAIL(VC_ERR_ARG, "text_create: kind must be VC_TEXT_T5 or VC_TEXT_CLIP, got %d", c.kind);
  if (c.vocab_size <= 0 || c.num_layers <= 0 || c.num_layers > 4096 || c.num_heads <= 0 || c.d_model <= 0 || c.d_ff <= 0)
    FAIL(VC_ERR_ARG, "text_create: vocab_size, d_model, d_ff, num_layers and num_heads must be positive");
  // d_model, d_ff and the head width are the K of a GEMM (64 per K-tile); the row norms hold a row of up to 4096 in registers
  if (c.d_model % 64 || c.d_model > 4096 || c.d_ff % 64) FAIL(VC_ERR_ARG, "text_create: d_model = %d (<= 4096) and d_ff = %d must be multiples of 64", c.d_model, c.d_ff);
  int dh = c.d_kv;
  if (c.kind == VC_TEXT_CLIP) {
    if (c.d_model % c.num_heads) FAIL(VC_ERR_ARG, "text_create: d_model = %d is not a multiple of num_heads = %d", c.d_model, c.num_heads);
    dh = c.d_model / c.num_heads;
    if (c.d_kv != 0 && c.d_kv != dh) FAIL(VC_ERR_ARG, "text_create: a CLIP head is d_model / num_heads = %d wide (d_kv: 0 or that), got %d", dh, c.d_kv);
    if (c.max_positions <= 0 || c.max_positions > 16384) FAIL(VC_ERR_ARG, "text_create: max_positions must be 1..16384, got %d", c.max_positions);
  } else {
    if (c.num_buckets < 4 || c.num_buckets % 2 || c.num_buckets > 4 * (VC_T5_MAX_STEPS + 1) || c.max_distance <= c.num_buckets / 4)
      FAIL(VC_ERR_ARG, "text_create: num_buckets = %d must be even in 4..%d and max_distance = %d above num_buckets / 4", c.num_buckets,
           4 * (VC_T5_MAX_STEPS + 1), c.max_distance);
  }
  if (dh <= 0 || dh % 64 || (int64_t)c.num_heads * dh > (1 << 20)) FAIL(VC_ERR_ARG, "text_create: the head width %d must be a positive multiple of 64", dh);
  if (!(c.eps > 0.0f) || !isfinite(c.eps)) FAIL(VC_ERR_ARG, "text_create: eps must be positive and finite");
  Text* v = new Text();
  v->cfg = c;
  v->D = c.d_model; v->H = c.num_heads; v->dh = dh; v->F = c.d_ff;
  build_tree(*v);
  *handle = v;
  return VC_OK;
}

int vc_text_destroy_impl(void* handle, char* err, int errlen) {
  HANDLE(Text, v, "text");
  v.plans.clear();
  delete &v;
  return VC_OK;
}

int vc_text_weight_name_impl(void* handle, int32_t index, char* name, int32_t namelen, char* err, int errlen) {
  HANDLE(Text, v, "text");
  if (index < 0 || index >= (int)v.t.size()) FAIL(VC_ERR_ARG, "text_weight_name: index %d outside 0..%d", index, (int)v.t.size() - 1);
  if (!name || namelen <= (int)v.t[index].key.size()) FAIL(VC_ERR_ARG, "text_weight_name: name buffer too small");
  strcpy(name, v.t[index].key.c_str());
  return VC_OK;
}

int vc_text_bind_tensor_impl(void* handle, const char* key, const void* ptr, const int64_t* shape, int32_t ndim, char* err, int errlen) {
  HANDLE(Text, v, "text");
  if (!key) FAIL(VC_ERR_ARG, "text_bind_tensor: null key");
  auto it = v.by_key.find(key);
  if (it == v.by_key.end()) FAIL(VC_ERR_ARG, "text_bind_tensor: unknown key '%s'", key);
  Tensor& t = v.t[it->second];
  if (!ptr || !shape) FAIL(VC_ERR_ARG, "text_bind_tensor: null pointer or shape for '%s'", key);
  if (ndim != t.ndim || shape[0] != t.shape[0] || (t.ndim == 2 && shape[1] != t.shape[1])) {
    if (t.ndim == 2) FAIL(VC_ERR_ARG, "text_bind_tensor: '%s' has shape [%ld, %ld]", key, (long)t.shape[0], (long)t.shape[1]);
    FAIL(VC_ERR_ARG, "text_bind_tensor: '%s' has shape [%ld]", key, (long)t.shape[0]);
  }
  if ((uintptr_t)ptr & 15) FAIL(VC_ERR_ARG, "text_bind_tensor: '%s' must be 16-byte aligned", key);
  v.plans.clear();           // a captured plan holds the old pointer
  t.p = (const bf16_t*)ptr;
  if (it->second == v.rel) v.bias_ready = false;
  return VC_OK;
}

int vc_text_workspace_bytes_impl(void* handle, int32_t L, int64_t* bytes, char* err, int errlen) {
  HANDLE(Text, v, "text");
  if (!bytes) FAIL(VC_ERR_ARG, "text_workspace_bytes: null result pointer");
  TRY(check_len(v, L, e, "text_workspace_bytes"));
  char* none[NBUF];
  *bytes = carve(v, L, nullptr, none);
  return VC_OK;
}

int vc_text_prepare_impl(void* handle, int32_t L, void* workspace, int64_t workspace_bytes, hipStream_t s, char* err, int errlen) {
  HANDLE(Text, v, "text");
  TRY(check_len(v, L, e, "text_prepare"));
  if (!aligned256(workspace)) FAIL(VC_ERR_ARG, "text_prepare: the workspace must be a 256-byte aligned device pointer");
  char* ptr[NBUF];
  const int64_t need = carve(v, L, (char*)workspace, ptr);
  if (workspace_bytes < need) FAIL(VC_ERR_ARG, "text_prepare: workspace too small (%ld < %ld bytes)", (long)workspace_bytes, (long)need);
  v.prepared = false;
  HIP(hipMemsetD16Async((hipDeviceptr_t)ptr[ONES], 0x3F80, (size_t)v.D, s), "hipMemsetD16Async");   // bf16 1.0
  memcpy(v.ptr, ptr, sizeof(ptr));
  v.L = L; v.R = v.cfg.kind == VC_TEXT_T5 ? L : (L + 63) / 64 * 64; v.base = (char*)workspace;
  v.bias_ready = false;
  if (v.cfg.kind == VC_TEXT_T5 && v.t[v.rel].p) TRY(build_bias(v, s, e));     // not bound yet: the first encode builds it
  v.prepared = true;
  return VC_OK;
}

int vc_text_encode_impl(void* handle, const int32_t* ids, int32_t n_prompts, void* hidden, void* pooled, hipStream_t s, char* err, int errlen) {
  HANDLE(Text, v, "text");
  const bool t5 = v.cfg.kind == VC_TEXT_T5;
  if (!ids || n_prompts <= 0) FAIL(VC_ERR_ARG, "text_encode: null ids or no prompt");
  if (t5 && pooled) FAIL(VC_ERR_ARG, "text_encode: a T5 handle has no pooled output (pooled must be NULL)");
  if (!hidden && !pooled) FAIL(VC_ERR_ARG, "text_encode: hidden and pooled are both NULL");
  for (const Tensor& t : v.t)
    if (t.read && !t.p) FAIL(VC_ERR_STATE, "text_encode: tensor '%s' is not bound", t.key.c_str());
  if (!v.prepared) FAIL(VC_ERR_STATE, "text_encode: call vc_text_prepare first");
  if (t5 && !v.bias_ready) TRY(build_bias(v, s, e));
  const Text::Key k{v.base, v.L, s};
  const int64_t row = (int64_t)v.D * 2;
  for (int i = 0; i < n_prompts; ++i) {        // the copies stay outside the graph: it is a chain of kernel nodes over resident buffers
    HIP(hipMemcpyAsync(v.ptr[IDS], ids + (int64_t)i * v.L, (size_t)v.L * 4, hipMemcpyDeviceToDevice, s), "hipMemcpyAsync(ids)");
    TRY(run_captured(v.plans, v.warmed, k, k.L, e, [&] {   // one prompt's launches
      Run r{v, s, e};
      return t5 ? t5_plan(r) : clip_plan(r);
    }));
    if (hidden) HIP(hipMemcpyAsync((char*)hidden + i * v.L * row, v.ptr[OUT], (size_t)(v.L * row), hipMemcpyDeviceToDevice, s), "hipMemcpyAsync(hidden)");
    if (pooled) HIP(hipMemcpyAsync((char*)pooled + i * row, v.ptr[POOL], (size_t)row, hipMemcpyDeviceToDevice, s), "hipMemcpyAsync(pooled)");
  }
  return VC_OK;
}

const VcTextConfig* vc_text_config_impl(void* handle) { return handle ? &((Text*)handle)->cfg : nullptr; }   // grid_engine.hip reads the geometry
int vc_text_plan_count_impl(void* handle) { return handle ? (int)((Text*)handle)->plans.size() : -1; }
