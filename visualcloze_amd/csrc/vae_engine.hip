// Autoencoder handle of include/vcloze_hip.h: AutoEncoder.decode / AutoEncoder.encode (models/modules/autoencoder.py:277-311) as
// launch plans over the kernels of this library.  Host code only: it ORDERS launches - the order visualcloze_amd/vae.py spells in
// Python over the op-level ABI (the parity twin: same kernels, same order, same bits) - once per (geometry, direction, pointers)
// under stream capture.  What vae.py does in torch between two launches is here
//   the weight re-layout ([O, I, k, k] -> [O_pad8, k*k*I_pad64] bf16) and the bf16 casts   two kernels of vae.hip, at bind time
//   the zero row behind every activation map, the zero pads of the attention operands      zero_fill_kernel launches of the plan
//   the residual gate of ones                                                               one 16-bit memset at prepare time
//
// Workspace (caller's device memory) per half (encoder / decoder), bf16 unless noted, named like vae.py's scratch pool; HW = the
// largest map, every "map" carries one extra zero row (the source of vc_conv3x3's out-of-image taps):
//   ZIN  map [HW, pad64(in)]    the NHWC input          XA / XB  maps [HW, C]   the residual stream, ping-pong
//   T0 / T2  maps               GroupNorm outputs       T1 / T3  [HW, C]        conv1 output / nin_shortcut output
//   GN   f32                    GroupNorm statistics    AQ AV AK AS AVT AO      mid-block attention: q, v, k, scores, V^T, P.V
//   YOUT [HW, pad8(out)]        conv_out's output       LAT [z, h, w]           the NCHW latent beside a token-form argument
//   ONES [max C]                the gate of `x + h` (autoencoder.py:82) for the fused residual epilogue
#include "common.h"
#include "vcloze_internal.h"
#include "engine_core.h"
#include <math.h>
#include <string.h>
#include <string>
#include <unordered_map>
#include <vector>

namespace {

constexpr int GN_GROUPS = 32;          // nn.GroupNorm(32, C, eps=1e-6), autoencoder.py:21-22
constexpr float GN_EPS = 1e-6f;

// one module with parameters: an nn.Conv2d (k = 3 or 1) or an nn.GroupNorm
struct Mod {
  std::string name;
  int k = 0;                 // 3, 1, or 0 = GroupNorm
  int cin = 0, cout = 0;     // GroupNorm: cout = C
  void* mem = nullptr;       // the handle's device copy: w, then b
  const bf16_t* w = nullptr; // conv: [pad8(cout), k*k*pad64(cin)]; GroupNorm: gamma [C]
  const bf16_t* b = nullptr; // conv: [pad8(cout)]; GroupNorm: beta [C]
};
struct Res { int cin = 0, cout = 0, norm1 = -1, conv1 = -1, norm2 = -1, conv2 = -1, nin = -1; };
struct Attn { int C = 0, norm = -1, q = -1, k = -1, v = -1, proj = -1; };
struct Level { std::vector<Res> blocks; int resample = -1; };
struct Half {
  int first = 0, last = 0;   // its modules are mods[first .. last)
  int conv_in = -1, norm_out = -1, conv_out = -1;
  std::vector<Level> levels; // by level index, as the state dict names them
  Res mid1, mid2;
  Attn attn;
};

enum BufId { ZIN, XA, XB, T0, T1, T2, T3, GN, AQ, AV, AK, AS, AVT, AO, YOUT, LAT, ONES, NBUF };
struct Side {
  char* ptr[NBUF] = {};
  int64_t bytes[NBUF] = {};
};

enum { DIR_ENCODE = 0, DIR_DECODE = 1 };

struct Vae {
  VcVaeConfig cfg{};
  int nres = 0, f = 1;
  std::vector<Mod> mods;
  std::unordered_map<std::string, int> by_name;
  Half enc, dec;
  // prepared geometry + workspace carve-up
  bool prepared = false;
  int H = 0, W = 0, which = 0;
  char* base = nullptr;
  Side side[2];              // [DIR_ENCODE], [DIR_DECODE]
  // captured plans, most recently used first
  struct Key {
    char* base; int H, W, which /* the carve-up of base depends on it */, dir, form, pix_f32; const void* in; const void* noise; void* out; int64_t ld; int col0; hipStream_t s;
    bool operator==(const Key& o) const {
      return base == o.base && H == o.H && W == o.W && which == o.which && dir == o.dir && form == o.form && pix_f32 == o.pix_f32 && in == o.in &&
             noise == o.noise && out == o.out && ld == o.ld && col0 == o.col0 && s == o.s;
    }
  };
  PlanCache<Key, hipGraphExec_t, 8, DropExec> plans;
  // plan shapes that have run un-captured once on this handle (H, W, dir, form, pix_f32, noise given): the run that sets the
  // kernels' attributes is needed once per set of launches, not once per set of argument pointers
  struct Shape {
    int H, W, dir, form, pix_f32, noise;
    bool operator==(const Shape& o) const { return H == o.H && W == o.W && dir == o.dir && form == o.form && pix_f32 == o.pix_f32 && noise == o.noise; }
  };
  std::vector<Shape> warmed;
};

// ---------------------------------------------------------------- the module tree (autoencoder.py:109-259), in state-dict order
int add_mod(Vae& v, const std::string& name, int k, int cin, int cout) {
  Mod m;
  m.name = name; m.k = k; m.cin = cin; m.cout = cout;
  v.mods.push_back(m);
  v.by_name[name] = (int)v.mods.size() - 1;
  return (int)v.mods.size() - 1;
}
Res add_res(Vae& v, const std::string& p, int cin, int cout) {     // ResnetBlock, :55-82
  Res r;
  r.cin = cin; r.cout = cout;
  r.norm1 = add_mod(v, p + ".norm1", 0, cin, cin);
  r.conv1 = add_mod(v, p + ".conv1", 3, cin, cout);
  r.norm2 = add_mod(v, p + ".norm2", 0, cout, cout);
  r.conv2 = add_mod(v, p + ".conv2", 3, cout, cout);
  if (cin != cout) r.nin = add_mod(v, p + ".nin_shortcut", 1, cin, cout);
  return r;
}
void add_mid(Vae& v, Half& h, const std::string& p, int C) {       // block_1, attn_1 (AttnBlock, :25-52), block_2
  h.mid1 = add_res(v, p + ".mid.block_1", C, C);
  h.attn.C = C;
  h.attn.norm = add_mod(v, p + ".mid.attn_1.norm", 0, C, C);
  h.attn.q = add_mod(v, p + ".mid.attn_1.q", 1, C, C);
  h.attn.k = add_mod(v, p + ".mid.attn_1.k", 1, C, C);
  h.attn.v = add_mod(v, p + ".mid.attn_1.v", 1, C, C);
  h.attn.proj = add_mod(v, p + ".mid.attn_1.proj_out", 1, C, C);
  h.mid2 = add_res(v, p + ".mid.block_2", C, C);
}
void build_tree(Vae& v) {
  const VcVaeConfig& c = v.cfg;
  const int n = c.n_ch_mult;
  char nm[96];
  {                          // Encoder, :109-157: level i maps ch * in_ch_mult[i] -> ch * ch_mult[i]
    Half& h = v.enc;
    h.first = (int)v.mods.size();
    h.conv_in = add_mod(v, "encoder.conv_in", 3, c.in_channels, c.ch);
    for (int i = 0; i < n; ++i) {
      const int cin = c.ch * (i == 0 ? 1 : c.ch_mult[i - 1]), cout = c.ch * c.ch_mult[i];
      Level l;
      for (int j = 0; j < c.num_res_blocks; ++j) {
        snprintf(nm, sizeof(nm), "encoder.down.%d.block.%d", i, j);
        l.blocks.push_back(add_res(v, nm, j == 0 ? cin : cout, cout));
      }
      if (i != n - 1) {
        snprintf(nm, sizeof(nm), "encoder.down.%d.downsample.conv", i);
        l.resample = add_mod(v, nm, 3, cout, cout);
      }
      h.levels.push_back(l);
    }
    const int top = c.ch * c.ch_mult[n - 1];
    add_mid(v, h, "encoder", top);
    h.norm_out = add_mod(v, "encoder.norm_out", 0, top, top);
    h.conv_out = add_mod(v, "encoder.conv_out", 3, top, 2 * c.z_channels);
    h.last = (int)v.mods.size();
  }
  {                          // Decoder, :183-235: the walk goes from the last level down to 0, the state dict is by level index
    Half& h = v.dec;
    h.first = (int)v.mods.size();
    const int top = c.ch * c.ch_mult[n - 1];
    h.conv_in = add_mod(v, "decoder.conv_in", 3, c.z_channels, top);
    add_mid(v, h, "decoder", top);
    for (int i = 0; i < n; ++i) {
      const int cout = c.ch * c.ch_mult[i];
      const int cin = i == n - 1 ? top : c.ch * c.ch_mult[i + 1];     // the previous level of the walk
      Level l;
      for (int j = 0; j < c.num_res_blocks + 1; ++j) {
        snprintf(nm, sizeof(nm), "decoder.up.%d.block.%d", i, j);
        l.blocks.push_back(add_res(v, nm, j == 0 ? cin : cout, cout));
      }
      if (i != 0) {
        snprintf(nm, sizeof(nm), "decoder.up.%d.upsample.conv", i);
        l.resample = add_mod(v, nm, 3, cout, cout);
      }
      h.levels.push_back(l);
    }
    h.norm_out = add_mod(v, "decoder.norm_out", 0, c.ch * c.ch_mult[0], c.ch * c.ch_mult[0]);
    h.conv_out = add_mod(v, "decoder.conv_out", 3, c.ch * c.ch_mult[0], c.out_ch);
    h.last = (int)v.mods.size();
  }
}

// ---------------------------------------------------------------- the plan
// dry: nothing is launched, buffer requests only record their sizes (vc_vae_workspace_bytes / the carve-up of vc_vae_prepare)
struct Run {
  Vae& v; Side& sd; bool dry; hipStream_t s; Err e;
};

int buf(Run& r, int id, int64_t bytes, void** out) {
  Err e = r.e;
  if (r.dry) {
    if (bytes > r.sd.bytes[id]) r.sd.bytes[id] = bytes;
    *out = nullptr;
    return VC_OK;
  }
  if (!r.sd.ptr[id] || bytes > r.sd.bytes[id]) FAIL(VC_ERR_STATE, "vae: workspace buffer %d holds %ld bytes, the plan needs %ld", id, (long)r.sd.bytes[id], (long)bytes);
  *out = r.sd.ptr[id];
  return VC_OK;
}
int zero(Run& r, void* p, int64_t offset, int64_t bytes) {     // bytes [offset, offset + bytes) of buffer p
  if (r.dry || bytes <= 0) return VC_OK;
  return vc_zero_fill_launch((char*)p + offset, bytes, r.s, r.e.buf, r.e.len);
}
// activation map [HW + 1, C]: rows 0..HW-1 are the pixels, row HW the zero row (writers only touch rows < HW)
int act(Run& r, int id, int64_t HW, int C, bf16_t** out) {
  void* p = nullptr;
  TRY(buf(r, id, (HW + 1) * C * 2, &p));
  *out = (bf16_t*)p;
  return zero(r, p, HW * C * 2, (int64_t)C * 2);
}
int plain(Run& r, int id, int64_t elems, bf16_t** out) {
  void* p = nullptr;
  TRY(buf(r, id, elems * 2, &p));
  *out = (bf16_t*)p;
  return VC_OK;
}
int ones(Run& r, int n, bf16_t** out) { return plain(r, ONES, n, out); }

// out[H*W, pad8(cout)] = conv3x3(x) (+ res); x: a map with C channels per pixel and its zero row
int conv3(Run& r, int mi, const bf16_t* x, int C, int H, int W, bf16_t* out, int mode, bool with_res = false, const bf16_t* res = nullptr,
          int64_t ldres = 0) {
  const Mod& m = r.v.mods[mi];
  const int O = pad_to(m.cout, 8);
  bf16_t* gate = nullptr;
  if (with_res) TRY(ones(r, O, &gate));          // sized in a dry run too, where every pointer is null
  if (r.dry) return VC_OK;
  return vc_conv3x3_launch(x, m.w, m.b, out, O, with_res ? res : nullptr, ldres, gate, H, W, C, O, mode, r.s, r.e.buf, r.e.len);
}
int gemm(Run& r, const void* A, int64_t lda, const void* Wm, int64_t ldw, const void* bias, void* C, int64_t ldc, int M, int N, int K,
         const void* res, int64_t ldres, const void* gate) {
  if (r.dry) return VC_OK;
  VcGemmArgs a;
  memset(&a, 0, sizeof(a));
  a.nprob = 1;
  a.epi = res ? VC_EPI_GATE_RES : VC_EPI_BIAS;
  VcGemmProblem& p = a.p[0];
  p.A = A; p.W = Wm; p.bias = bias; p.C = C; p.res = res; p.gate = gate;
  p.lda = lda; p.ldw = ldw; p.ldc = ldc; p.ldres = ldres;
  p.M = M; p.N = N; p.K = K; p.rows_per_batch = M;
  return vc_gemm_launch(a, 0, r.s, r.e.buf, r.e.len);
}
// 1x1 convolution = GEMM over the pixel rows
int conv1(Run& r, int mi, const bf16_t* x, int M, bf16_t* out, bool with_res = false, const bf16_t* res = nullptr) {
  const Mod& m = r.v.mods[mi];
  const int O = pad_to(m.cout, 8), K = pad_to(m.cin, 64);
  bf16_t* gate = nullptr;
  if (with_res) TRY(ones(r, O, &gate));
  return gemm(r, x, m.cin, m.w, K, m.b, out, O, M, O, m.cin, with_res ? res : nullptr, O, gate);
}
int norm(Run& r, int mi, const bf16_t* x, bf16_t* y, int64_t HW, int swish) {
  const Mod& m = r.v.mods[mi];
  const int64_t bytes = ((HW + 127) / 128 + 1) * 2 * GN_GROUPS * 4;
  void* sc = nullptr;
  TRY(buf(r, GN, bytes, &sc));
  if (r.dry) return VC_OK;
  return vc_groupnorm_launch(x, m.w, m.b, y, sc, bytes, HW, m.cout, GN_GROUPS, GN_EPS, swish, r.s, r.e.buf, r.e.len);
}

// ResnetBlock.forward (:70-82).  x: a map [HW + 1, cin]; *out: the map `tag` [HW + 1, cout]
int resnet(Run& r, const Res& b, const bf16_t* x, int H, int W, int tag, bf16_t** out) {
  const int64_t HW = (int64_t)H * W;
  bf16_t *t, *h, *t2, *o;
  TRY(act(r, T0, HW, b.cin, &t));
  TRY(norm(r, b.norm1, x, t, HW, 1));
  TRY(plain(r, T1, HW * b.cout, &h));
  TRY(conv3(r, b.conv1, t, b.cin, H, W, h, 0));
  TRY(act(r, T2, HW, b.cout, &t2));
  TRY(norm(r, b.norm2, h, t2, HW, 1));
  const bf16_t* res = x;
  if (b.cin != b.cout) {
    bf16_t* sc;
    TRY(plain(r, T3, HW * b.cout, &sc));
    TRY(conv1(r, b.nin, x, (int)HW, sc));
    res = sc;
  }
  TRY(act(r, tag, HW, b.cout, &o));
  TRY(conv3(r, b.conv2, t2, b.cout, H, W, o, 0, true, res, b.cout));
  *out = o;
  return VC_OK;
}

// AttnBlock.forward (:32-52): one head, head_dim = C, as two GEMMs around vc_softmax_rows
int attention(Run& r, const Attn& a, const bf16_t* x, int64_t L, int tag, bf16_t** out) {
  const int C = a.C;
  const int64_t Lk = (L + 7) / 8 * 8, Lp = (L + 63) / 64 * 64;    // N of the S GEMM / K of the P.V GEMM; the pads stay zero
  bf16_t *t, *q, *v, *k, *s, *vt, *o, *y;
  TRY(plain(r, T0, L * C, &t));
  TRY(norm(r, a.norm, x, t, L, 0));
  TRY(plain(r, AQ, L * C, &q));
  TRY(plain(r, AV, L * C, &v));
  TRY(plain(r, AK, Lk * C, &k));
  if (Lk != L) TRY(zero(r, k, L * C * 2, (Lk - L) * C * 2));           // zero key rows -> zero score columns L..Lk-1
  TRY(conv1(r, a.q, t, (int)L, q));
  TRY(conv1(r, a.k, t, (int)L, k));
  TRY(conv1(r, a.v, t, (int)L, v));
  TRY(plain(r, AS, L * Lp, &s));
  if (Lp != L) TRY(zero(r, s, 0, L * Lp * 2));
  TRY(gemm(r, q, C, k, C, nullptr, s, Lp, (int)L, (int)Lk, C, nullptr, 0, nullptr));              // S = Q K^T  [L, L]
  if (!r.dry) TRY(vc_softmax_rows_launch(s, Lp, (int)L, (int)L, (float)pow((double)C, -0.5), nullptr, 0, 0, r.s, r.e.buf, r.e.len));
  TRY(plain(r, AVT, C * Lp, &vt));
  if (Lp != L) TRY(zero(r, vt, 0, C * Lp * 2));
  if (!r.dry) TRY(vc_transpose_launch(v, C, vt, Lp, (int)L, C, r.s, r.e.buf, r.e.len));
  TRY(plain(r, AO, L * C, &o));
  TRY(gemm(r, s, Lp, vt, Lp, nullptr, o, C, (int)L, C, (int)Lp, nullptr, 0, nullptr));            // O = P V
  TRY(act(r, tag, L, C, &y));
  TRY(conv1(r, a.proj, o, (int)L, y, true, x));
  *out = y;
  return VC_OK;
}

struct Flip {                // the residual stream alternates between XB and XA ("xb" first, as vae.py's flip list)
  int k = 0;
  int next() { return (k++ & 1) ? XA : XB; }
};

// Decoder.forward (:237-259) behind `z / scale_factor + shift_factor` (:306-307)
int decode_plan(Run& r, int H, int W, const void* latent, int form, int64_t ld, int col0, void* pixels, int pix_f32) {
  Vae& v = r.v;
  const VcVaeConfig& c = v.cfg;
  const Half& d = v.dec;
  int h = H / v.f, w = W / v.f;
  const int Z = c.z_channels, Zp = pad_to(Z, 64);
  int src_f32 = form == VC_VAE_LATENT_F32;
  if (form == VC_VAE_TOKENS) {
    bf16_t* lat;
    TRY(plain(r, LAT, (int64_t)Z * h * w, &lat));
    if (!r.dry) TRY(vc_unpack_latent_launch(latent, ld, col0, lat, Z, h, w, r.s, r.e.buf, r.e.len));
    latent = lat;
  }
  bf16_t *x0, *cur;
  TRY(act(r, ZIN, (int64_t)h * w, Zp, &x0));
  if (!r.dry) TRY(vc_nchw_to_nhwc_launch(latent, src_f32, x0, Z, Zp, (int64_t)h * w, c.scale_factor, c.shift_factor, r.s, r.e.buf, r.e.len));
  TRY(act(r, XA, (int64_t)h * w, v.mods[d.conv_in].cout, &cur));
  TRY(conv3(r, d.conv_in, x0, Zp, h, w, cur, 0));
  Flip fl;
  TRY(resnet(r, d.mid1, cur, h, w, fl.next(), &cur));
  TRY(attention(r, d.attn, cur, (int64_t)h * w, fl.next(), &cur));
  TRY(resnet(r, d.mid2, cur, h, w, fl.next(), &cur));
  int C = d.attn.C;
  for (int i = c.n_ch_mult - 1; i >= 0; --i) {
    for (const Res& b : d.levels[i].blocks) { TRY(resnet(r, b, cur, h, w, fl.next(), &cur)); C = b.cout; }
    if (i != 0) {            // Upsample (:98-106): nearest 2x folded into the convolution's gather
      h *= 2; w *= 2;
      bf16_t* nxt;
      TRY(act(r, fl.next(), (int64_t)h * w, C, &nxt));
      TRY(conv3(r, d.levels[i].resample, cur, C, h, w, nxt, 1));
      cur = nxt;
    }
  }
  const int64_t HW = (int64_t)h * w;
  const int Op = pad_to(c.out_ch, 8);
  bf16_t *t, *y;
  TRY(act(r, T0, HW, C, &t));
  TRY(norm(r, d.norm_out, cur, t, HW, 1));
  TRY(plain(r, YOUT, HW * Op, &y));
  TRY(conv3(r, d.conv_out, t, C, h, w, y, 0));
  if (!r.dry) TRY(vc_nhwc_to_nchw_launch(y, pixels, pix_f32, c.out_ch, Op, HW, r.s, r.e.buf, r.e.len));
  return VC_OK;
}

// Encoder.forward (:159-180), DiagonalGaussian (:268-275) and `scale_factor * (z - shift_factor)` (:301-304)
int encode_plan(Run& r, int H, int W, const void* pixels, int pix_f32, const void* noise, void* latent, int form, int64_t ld, int col0) {
  Vae& v = r.v;
  const VcVaeConfig& c = v.cfg;
  const Half& d = v.enc;
  int h = H, w = W;
  const int Ip = pad_to(c.in_channels, 64);
  bf16_t *x0, *cur;
  TRY(act(r, ZIN, (int64_t)h * w, Ip, &x0));
  if (!r.dry) TRY(vc_nchw_to_nhwc_launch(pixels, pix_f32, x0, c.in_channels, Ip, (int64_t)h * w, 1.0f, 0.0f, r.s, r.e.buf, r.e.len));
  TRY(act(r, XA, (int64_t)h * w, c.ch, &cur));
  TRY(conv3(r, d.conv_in, x0, Ip, h, w, cur, 0));
  Flip fl;
  int C = c.ch;
  for (int i = 0; i < c.n_ch_mult; ++i) {
    for (const Res& b : d.levels[i].blocks) { TRY(resnet(r, b, cur, h, w, fl.next(), &cur)); C = b.cout; }
    if (i != c.n_ch_mult - 1) {          // Downsample (:85-95): pad (0,1,0,1) + stride 2, folded into the gather
      h /= 2; w /= 2;
      bf16_t* nxt;
      TRY(act(r, fl.next(), (int64_t)h * w, C, &nxt));
      TRY(conv3(r, d.levels[i].resample, cur, C, h, w, nxt, 2));
      cur = nxt;
    }
  }
  TRY(resnet(r, d.mid1, cur, h, w, fl.next(), &cur));
  TRY(attention(r, d.attn, cur, (int64_t)h * w, fl.next(), &cur));
  TRY(resnet(r, d.mid2, cur, h, w, fl.next(), &cur));
  const int64_t HW = (int64_t)h * w;
  const int Z = c.z_channels, Mp = pad_to(2 * Z, 8);
  bf16_t *t, *mom;
  TRY(act(r, T0, HW, C, &t));
  TRY(norm(r, d.norm_out, cur, t, HW, 1));
  TRY(plain(r, YOUT, HW * Mp, &mom));
  TRY(conv3(r, d.conv_out, t, C, h, w, mom, 0));
  void* z = latent;
  if (form == VC_VAE_TOKENS) {
    bf16_t* lat;
    TRY(plain(r, LAT, (int64_t)Z * HW, &lat));
    z = lat;
  }
  if (!r.dry) TRY(vc_gaussian_sample_launch(mom, Mp, noise, z, Z, HW, c.scale_factor, c.shift_factor, r.s, r.e.buf, r.e.len));
  if (form == VC_VAE_TOKENS && !r.dry) TRY(vc_pack_latent_launch(z, latent, Z, h, w, ld, col0, r.s, r.e.buf, r.e.len));
  return VC_OK;
}

int check_size(const Vae& v, int H, int W, int which, Err e, const char* what) {
  if (which < 1 || which > 3) FAIL(VC_ERR_ARG, "%s: which must be VC_VAE_ENCODER, VC_VAE_DECODER or both, got %d", what, which);
  if (H <= 0 || W <= 0 || H % v.f || W % v.f || H >= 65536 || W >= 65536)
    FAIL(VC_ERR_ARG, "%s: image size %dx%d must be positive multiples of %d below 65536", what, H, W, v.f);
  return VC_OK;
}

// the buffer sizes of the chosen halves at (H, W): a dry run of both plans in their widest forms
int size_sides(Vae& v, int H, int W, int which, Side out[2], Err e) {
  for (int dir = 0; dir < 2; ++dir) {
    out[dir] = Side{};
    if (!(which & (dir == DIR_ENCODE ? VC_VAE_ENCODER : VC_VAE_DECODER))) continue;
    Run r{v, out[dir], true, nullptr, e};
    if (dir == DIR_ENCODE) TRY(encode_plan(r, H, W, nullptr, 0, nullptr, nullptr, VC_VAE_TOKENS, 0, 0));
    else TRY(decode_plan(r, H, W, nullptr, VC_VAE_TOKENS, 0, 0, nullptr, 0));
  }
  return VC_OK;
}
int64_t carve(Side sides[2], char* base) {
  Carver c{base};
  for (int dir = 0; dir < 2; ++dir)
    for (int i = 0; i < NBUF; ++i) sides[dir].ptr[i] = c.bytes(sides[dir].bytes[i]);
  return c.off;
}

// the checks every decode / encode call makes before anything is launched
int ready(const Vae& v, int dir, Err e, const char* what) {
  const Half& h = dir == DIR_ENCODE ? v.enc : v.dec;
  for (int i = h.first; i < h.last; ++i)
    if (!v.mods[i].w) FAIL(VC_ERR_STATE, "%s: weight '%s.weight' is not bound", what, v.mods[i].name.c_str());
  if (!v.prepared || !(v.which & (dir == DIR_ENCODE ? VC_VAE_ENCODER : VC_VAE_DECODER)))
    FAIL(VC_ERR_STATE, "%s: call vc_vae_prepare with %s first", what, dir == DIR_ENCODE ? "VC_VAE_ENCODER" : "VC_VAE_DECODER");
  return VC_OK;
}
int check_tokens(const Vae& v, int64_t ld, int col0, const void* tokens, Err e, const char* what) {
  const int h = v.H / v.f, w = v.W / v.f;
  if ((h | w) & 1) FAIL(VC_ERR_ARG, "%s: the token form needs an even latent size, got %dx%d", what, h, w);
  if (v.cfg.z_channels > 64) FAIL(VC_ERR_ARG, "%s: the token form packs at most 64 latent channels", what);
  if (ld % 8 || col0 % 8 || col0 < 0 || ld < col0 + 4 * v.cfg.z_channels || ((uintptr_t)tokens & 15))
    FAIL(VC_ERR_ARG, "%s: token rows need ld, col0 multiples of 8, ld >= col0 + %d and a 16-byte aligned base (ld=%ld col0=%d)", what,
         4 * v.cfg.z_channels, (long)ld, col0);
  return VC_OK;
}

}  // namespace

int vc_vae_create_impl(const VcVaeConfig* cfg, void** handle, char* err, int errlen) {
  Err e{err, errlen};
  if (!cfg || !handle) FAIL(VC_ERR_ARG, "vae_create: null argument");
  if (cfg->n_ch_mult < 1 || cfg->n_ch_mult > 8) FAIL(VC_ERR_ARG, "vae_create: n_ch_mult must be 1..8, got %d", cfg->n_ch_mult);
  if (cfg->in_channels <= 0 || cfg->out_ch <= 0 || cfg->z_channels <= 0 || cfg->num_res_blocks <= 0 || cfg->ch <= 0)
    FAIL(VC_ERR_ARG, "vae_create: channel counts and num_res_blocks must be positive");
  for (int i = 0; i < cfg->n_ch_mult; ++i) {
    const int64_t wd = (int64_t)cfg->ch * cfg->ch_mult[i];
    // a map's channels are the K of the next convolution (64 per K-tile) and GroupNorm(32)'s 8-channel chunks must divide 256
    if (cfg->ch_mult[i] <= 0 || wd % 64 || wd > 2048 || 256 % (wd / 8))
      FAIL(VC_ERR_ARG, "vae_create: ch * ch_mult[%d] = %ld must be 64, 128, 256, 512, 1024 or 2048", i, (long)wd);
  }
  if (!(cfg->scale_factor != 0.0f) || !isfinite(cfg->scale_factor) || !isfinite(cfg->shift_factor))
    FAIL(VC_ERR_ARG, "vae_create: scale_factor must be finite and non-zero, shift_factor finite");
  Vae* v = new Vae();
  v->cfg = *cfg;
  v->nres = cfg->n_ch_mult;
  v->f = 1 << (cfg->n_ch_mult - 1);
  build_tree(*v);
  *handle = v;
  return VC_OK;
}

int vc_vae_destroy_impl(void* handle, char* err, int errlen) {
  HANDLE(Vae, v, "vae");
  v.plans.clear();
  for (auto& m : v.mods) if (m.mem) (void)hipFree(m.mem);
  delete &v;
  return VC_OK;
}

int vc_vae_weight_name_impl(void* handle, int32_t index, char* name, int32_t namelen, char* err, int errlen) {
  HANDLE(Vae, v, "vae");
  if (index < 0 || index >= (int)v.mods.size()) FAIL(VC_ERR_ARG, "vae_weight_name: index %d outside 0..%d", index, (int)v.mods.size() - 1);
  if (!name || namelen <= (int)v.mods[index].name.size()) FAIL(VC_ERR_ARG, "vae_weight_name: name buffer too small");
  strcpy(name, v.mods[index].name.c_str());
  return VC_OK;
}

int vc_vae_bind_weight_impl(void* handle, const char* name, const void* w, const void* bias, int32_t is_f32, const int64_t* shape, int32_t ndim,
                            hipStream_t s, char* err, int errlen) {
  HANDLE(Vae, v, "vae");
  if (!name) FAIL(VC_ERR_ARG, "vae_bind_weight: null name");
  std::string key(name);
  if (key.size() > 7 && key.compare(key.size() - 7, 7, ".weight") == 0) key.resize(key.size() - 7);
  auto it = v.by_name.find(key);
  if (it == v.by_name.end()) FAIL(VC_ERR_ARG, "vae_bind_weight: unknown weight '%s'", name);
  Mod& m = v.mods[it->second];
  if (!w || !bias || !shape) FAIL(VC_ERR_ARG, "vae_bind_weight: null weight, bias or shape for '%s'", name);
  if (m.k == 0) {
    if (ndim != 1 || shape[0] != m.cout) FAIL(VC_ERR_ARG, "vae_bind_weight: '%s' is a GroupNorm affine of shape [%d]", name, m.cout);
  } else if (ndim != 4 || shape[0] != m.cout || shape[1] != m.cin || shape[2] != m.k || shape[3] != m.k) {
    FAIL(VC_ERR_ARG, "vae_bind_weight: '%s' is a convolution weight of shape [%d, %d, %d, %d]", name, m.cout, m.cin, m.k, m.k);
  }
  const int Op = m.k ? pad_to(m.cout, 8) : m.cout, Ip = pad_to(m.cin, 64), kk = m.k * m.k;
  const int64_t wbytes = align256(m.k ? (int64_t)Op * kk * Ip * 2 : (int64_t)m.cout * 2);
  void* mem = nullptr;
  HIP(hipMalloc(&mem, (size_t)(wbytes + align256((int64_t)Op * 2))), "hipMalloc");
  bf16_t* dw = (bf16_t*)mem;
  bf16_t* db = (bf16_t*)((char*)mem + wbytes);
  int rc = m.k ? vc_vae_weight_relayout_launch(w, is_f32 != 0, dw, m.cout, m.cin, kk, Op, Ip, s, err, errlen)
               : vc_vae_cast_pad_launch(w, is_f32 != 0, dw, m.cout, m.cout, s, err, errlen);
  if (rc == VC_OK) rc = vc_vae_cast_pad_launch(bias, is_f32 != 0, db, m.cout, Op, s, err, errlen);
  if (rc == VC_OK && hipStreamSynchronize(s) != hipSuccess) { snprintf(err, errlen, "vae_bind_weight: hipStreamSynchronize failed for '%s'", name); rc = VC_ERR_HIP; }
  if (rc != VC_OK) { (void)hipFree(mem); return rc; }
  v.plans.clear();           // a captured plan holds the old copy's pointers
  if (m.mem) (void)hipFree(m.mem);
  m.mem = mem; m.w = dw; m.b = db;
  return VC_OK;
}

int vc_vae_workspace_bytes_impl(void* handle, int32_t H, int32_t W, int32_t which, int64_t* bytes, char* err, int errlen) {
  HANDLE(Vae, v, "vae");
  if (!bytes) FAIL(VC_ERR_ARG, "vae_workspace_bytes: null result pointer");
  TRY(check_size(v, H, W, which, e, "vae_workspace_bytes"));
  Side sides[2];
  TRY(size_sides(v, H, W, which, sides, e));
  *bytes = carve(sides, nullptr);
  return VC_OK;
}

int vc_vae_prepare_impl(void* handle, int32_t H, int32_t W, int32_t which, void* workspace, int64_t workspace_bytes, hipStream_t s,
                        char* err, int errlen) {
  HANDLE(Vae, v, "vae");
  TRY(check_size(v, H, W, which, e, "vae_prepare"));
  if (!aligned256(workspace)) FAIL(VC_ERR_ARG, "vae_prepare: the workspace must be a 256-byte aligned device pointer");
  Side sides[2];
  TRY(size_sides(v, H, W, which, sides, e));
  const int64_t need = carve(sides, (char*)workspace);
  if (workspace_bytes < need) FAIL(VC_ERR_ARG, "vae_prepare: workspace too small (%ld < %ld bytes)", (long)workspace_bytes, (long)need);
  v.prepared = false;
  for (int dir = 0; dir < 2; ++dir)
    if (sides[dir].ptr[ONES])
      HIP(hipMemsetD16Async((hipDeviceptr_t)sides[dir].ptr[ONES], 0x3F80, (size_t)(sides[dir].bytes[ONES] / 2), s), "hipMemsetD16Async");   // bf16 1.0
  v.side[0] = sides[0]; v.side[1] = sides[1];
  v.H = H; v.W = W; v.which = which; v.base = (char*)workspace;
  v.prepared = true;
  return VC_OK;
}

int vc_vae_decode_impl(void* handle, const void* latent, int32_t form, int64_t ld, int32_t col0, void* pixels, int32_t pixels_is_f32,
                       hipStream_t s, char* err, int errlen) {
  HANDLE(Vae, v, "vae");
  if (!latent || !pixels) FAIL(VC_ERR_ARG, "vae_decode: null pointer");
  if (form != VC_VAE_LATENT_BF16 && form != VC_VAE_LATENT_F32 && form != VC_VAE_TOKENS) FAIL(VC_ERR_ARG, "vae_decode: unknown latent_form %d", form);
  TRY(ready(v, DIR_DECODE, e, "vae_decode"));
  if (form == VC_VAE_TOKENS) TRY(check_tokens(v, ld, col0, latent, e, "vae_decode"));
  else { ld = 0; col0 = 0; }
  pixels_is_f32 = pixels_is_f32 != 0;
  Vae::Key k{v.base, v.H, v.W, v.which, DIR_DECODE, form, pixels_is_f32, latent, nullptr, pixels, ld, col0, s};
  return run_captured(v.plans, v.warmed, k, Vae::Shape{k.H, k.W, k.dir, k.form, k.pix_f32, 0}, e, [&] {
    Run r{v, v.side[DIR_DECODE], false, s, e};
    return decode_plan(r, v.H, v.W, latent, form, ld, col0, pixels, pixels_is_f32);
  });
}

int vc_vae_encode_impl(void* handle, const void* pixels, int32_t pixels_is_f32, const void* noise, void* latent, int32_t form, int64_t ld,
                       int32_t col0, hipStream_t s, char* err, int errlen) {
  HANDLE(Vae, v, "vae");
  if (!latent || !pixels) FAIL(VC_ERR_ARG, "vae_encode: null pointer");
  if (form != VC_VAE_LATENT_BF16 && form != VC_VAE_TOKENS) FAIL(VC_ERR_ARG, "vae_encode: latent_form must be VC_VAE_LATENT_BF16 or VC_VAE_TOKENS, got %d", form);
  TRY(ready(v, DIR_ENCODE, e, "vae_encode"));
  if (form == VC_VAE_TOKENS) TRY(check_tokens(v, ld, col0, latent, e, "vae_encode"));
  else { ld = 0; col0 = 0; }
  pixels_is_f32 = pixels_is_f32 != 0;
  Vae::Key k{v.base, v.H, v.W, v.which, DIR_ENCODE, form, pixels_is_f32, pixels, noise, latent, ld, col0, s};
  return run_captured(v.plans, v.warmed, k, Vae::Shape{k.H, k.W, k.dir, k.form, k.pix_f32, noise != nullptr}, e, [&] {
    Run r{v, v.side[DIR_ENCODE], false, s, e};
    return encode_plan(r, v.H, v.W, pixels, pixels_is_f32, noise, latent, form, ld, col0);
  });
}

const VcVaeConfig* vc_vae_config_impl(void* handle) { return handle ? &((Vae*)handle)->cfg : nullptr; }   // grid_engine.hip reads the geometry
int vc_vae_plan_count_impl(void* handle) { return handle ? (int)((Vae*)handle)->plans.size() : -1; }
