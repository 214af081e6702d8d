// Host side of the fused TemporalUnet forward (unet_kernel.h holds its device code): the time-embedding table kernel, the weight
// packer, the handle (mmd_unet_create / destroy), the workspace and FLOP queries and the forward launches.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/mmd_amd.h"
#include "../../include/mmd_amd_debug.h"
#include "common.h"
#include "f16x2.h"
#include "guide_dev.h"
#include "unet_kernel.h"
#include "unet_spec.h"

namespace mmd {

// ----------------------------------------------------------------------------------------------------------------
// time embedding table: TimeEncoder (layers.py:232-258) + every block's cond_mlp (layers.py:337-341) for all integer t
// ----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float mish_exact(float y) {
  float sp = y > 20.f ? y : log1pf(expf(y));
  return y * tanhf(sp);
}

__global__ void time_table_kernel(TimeArgs a) {
  __shared__ float emb[32], h1[128], m[32];
  const int t = blockIdx.x, tid = threadIdx.x;   // 128 threads
  if (tid < 16) {
    const float f = expf((float)tid * -(logf(10000.f) / 15.f));
    const float v = (float)t * f;
    emb[tid] = sinf(v);
    emb[tid + 16] = cosf(v);
  }
  __syncthreads();
  {
    float s = a.b1[tid];
    for (int k = 0; k < 32; ++k) s += a.w1[tid * 32 + k] * emb[k];
    h1[tid] = mish_exact(s);
  }
  __syncthreads();
  if (tid < 32) {
    float s = a.b3[tid];
    for (int k = 0; k < 128; ++k) s += a.w3[tid * 128 + k] * h1[k];
    m[tid] = mish_exact(s);          // cond_mlp starts with Mish
  }
  __syncthreads();
  for (int r = 0; r < a.n_rtb; ++r)
    for (int c = tid; c < a.cout[r]; c += 128) {
      float s = a.cb[r][c];
      for (int k = 0; k < 32; ++k) s += a.cw[r][c * 32 + k] * m[k];
      a.table[(size_t)t * a.total + a.off[r] + c] = s;
    }
}

// ----------------------------------------------------------------------------------------------------------------
// host side: parameter spec, weight packing, forward orchestration
// ----------------------------------------------------------------------------------------------------------------

// the fused kernel's configuration: unet_input_dim 32, dim_mults (1, 2, 4) (every released checkpoint); anything else build_spec
// accepts runs layer by layer (unet_layers.hip)
static inline bool fused_config(int uid, int n_levels) { return uid == 32 && n_levels == 3; }

void launch_time_table(const TimeArgs& a, int T, hipStream_t st) { hipLaunchKernelGGL(time_table_kernel, dim3(T), dim3(128), 0, st, a); }

// downs.0's first conv (4 -> 32, k5) as ONE K = 32 chunk per n-tile: slot jj of lane (column n, lane group j) = tap 2 j + (jj >> 2),
// channel jj & 3 (taps >= 5: zero); is_res: the 1x1 residual conv [cout][4] on the centre tap's slots.  Interleaved column pairs.
static size_t pack_im2col4(std::vector<float>& blob, const float* w, int cout, bool is_res, const std::vector<float>& sc) {
  while (blob.size() % 4) blob.push_back(0.f);
  const size_t base = blob.size();
  const int tiles = cout / 16;
  blob.resize(base + ((size_t)tiles * 2 + 8) * 64 * 4, 0.f);
  uint16_t* out = reinterpret_cast<uint16_t*>(blob.data() + base);
  for (int t = 0; t < tiles; ++t)
    for (int lane = 0; lane < 64; ++lane)
      for (int jj = 0; jj < 8; ++jj) {
        const int n = (t / 2) * 32 + 2 * (lane & 15) + (t & 1), tap = 2 * (lane >> 4) + (jj >> 2), c = jj & 3;
        float v = 0.f;
        if (is_res) v = tap == 2 ? w[(size_t)n * 4 + c] : 0.f;
        else if (tap < 5) v = w[((size_t)n * 4 + c) * 5 + tap];
        uint16_t piece[2];
        f16_split_host(v, sc[n], piece);
        for (int q = 0; q < 2; ++q) out[(((size_t)t * 2 + q) * 64 + lane) * 8 + jj] = piece[q];
      }
  return base;
}
// ... of a 1x1 residual conv [cout][cin_full] chunk for the centre tap's extra streams: per n-tile [chunk kc][piece][lane]
static size_t pack_rd_res(std::vector<float>& blob, const float* wres, int cout, int cin_full, int c_lo, int cin_chunk,
                          bool pair_cols, const std::vector<float>& sc) {
  return pack_rd(blob, wres, cout, cin_full, c_lo, cin_chunk, 1, std::vector<int>{0}, false, pair_cols, sc);
}

// max over t of |time bias| per (RTB, channel): a host replica (double) of time_table_kernel, used only for the bound
// behind the static activation scales below (layers.py:232-258, 337-341)
static std::vector<std::vector<float>> time_bias_absmax(const float* const* tensors, const Spec& s, int T) {
  auto mish = [](double y) { return y * std::tanh(y > 20.0 ? y : std::log1p(std::exp(y))); };
  const float *w1 = tensors[s.t_time[0]], *b1 = tensors[s.t_time[1]], *w3 = tensors[s.t_time[2]], *b3 = tensors[s.t_time[3]];
  std::vector<std::vector<float>> mxv(s.rtb.size());
  for (size_t r = 0; r < s.rtb.size(); ++r) mxv[r].assign(s.rtb[r].cout, 0.f);
  for (int t = 0; t < T; ++t) {
    double emb[32], h1[128], m[32];
    for (int i = 0; i < 16; ++i) {
      const double f = std::exp((double)i * -(std::log(10000.0) / 15.0)), v = (double)t * f;
      emb[i] = std::sin(v); emb[i + 16] = std::cos(v);
    }
    for (int j = 0; j < 128; ++j) { double a = b1[j]; for (int k = 0; k < 32; ++k) a += (double)w1[j * 32 + k] * emb[k]; h1[j] = mish(a); }
    for (int j = 0; j < 32; ++j) { double a = b3[j]; for (int k = 0; k < 128; ++k) a += (double)w3[j * 128 + k] * h1[k]; m[j] = mish(a); }
    for (size_t r = 0; r < s.rtb.size(); ++r) {
      const float *cw = tensors[s.rtb[r].t_cw], *cb = tensors[s.rtb[r].t_cb];
      for (int c = 0; c < s.rtb[r].cout; ++c) {
        double a = cb[c];
        for (int k = 0; k < 32; ++k) a += (double)cw[c * 32 + k] * m[k];
        mxv[r][c] = fmaxf(mxv[r][c], (float)std::fabs(a));
      }
    }
  }
  return mxv;
}
// Static f16x2 input scale of a conv B: its input Mish(GroupNorm(.)) + time bias is bounded whatever the data --
// |x_hat| <= sqrt(N - 1) < 16 for a group of N = 256 values, Mish(y) in [-0.31, max(y, 0)] -- by B = max_c (max(0.31, 16
// |gamma_c| + |beta_c|) + max_t |tb_c(t)|); the power of two s = 2^(10 - floor(log2 B)) keeps every value below 2048 inside fp16
// and the typical ones (|x_hat| ~ 1) far above its denormals.
static float static_act_scale(const float* gamma, const float* beta, const std::vector<float>& tbmax, int c) {
  float B = 0.f;
  for (int i = 0; i < c; ++i) B = fmaxf(B, fmaxf(0.31f, 16.f * fabsf(gamma[i]) + fabsf(beta[i])) + tbmax[i] * 1.001f);
  if (!std::isfinite(B)) return 1.f;
  int ex;
  (void)frexpf(B, &ex);                      // B = f * 2^ex, f in [0.5, 1): floor(log2 B) = ex - 1
  return ldexpf(1.f, 10 - (ex - 1));
}


struct ConvW { size_t wbf, rec; };   // f16x2 pack; the conv's epilogue records (push_records)
struct RtbW { ConvW a, b; size_t res_bf, res_c1_bf; int tb_off; size_t a_c1_bf; float act_a; };
// a stage's tail conv: Downsample1d = one f16x2 pack, ConvTranspose1d = the two parity packs (wbf[1] = 0: none); its records
struct TailW { size_t rec, wbf[2]; };

// what the packer leaves behind: offsets (in floats) into the blob, and the static activation scales
struct UnetPack {
  int tb_total = 0;          // columns of a time-table row
  RtbW rtb[12];              // state_dict order: d00 d01 d10 d11 d20 d21 u00 u01 u10 u11 mid1 mid2
  TailW down[2], up[2];
  ConvW fin;
  size_t fin_w1 = 0, fin_rec1 = 0;               // final 1x1 conv: f16x2 pack (N padded to 16), records {bias, inverse scale / fin_act}
  float fin_act = 1.f;                           // static scale of the final block's activations
  size_t raw_time[4], raw_cw[12], raw_cb[12];    // the time MLP's and the cond_mlps' fp32 parameters (time_table_kernel)
  mmd_unet_record_table tables[32];              // directory of the record tables (mmd_debug_unet_pack)
  int n_tables = 0;
};

}  // namespace mmd

using namespace mmd;

struct mmd_unet_s {
  mmd::LayeredUnet* layered = nullptr;   // set: a configuration other than the fused kernel's; everything below is unused
  int T = 0;
  int precision = MMD_UNET_PRECISION_F32;   // mmd_unet_options.precision: F16 launches unet_f16.hip's kernels on the same blob
  int ns2_max = 512;         // unet_kernel<2> (two trajectories per workgroup) up to this batch size (mmd_unet_options.two_per_workgroup_max)
#ifndef MMD_NS1_MAX
#define MMD_NS1_MAX 256
#endif
  int ns1_max = MMD_NS1_MAX; // unet_kernel<1> (one trajectory per workgroup) up to this batch size (-DMMD_NS1_MAX=0: the A/B side build)
  size_t blob_bytes = 0;     // bytes of `blob` (mmd_unet_weight_bytes)
  float* blob = nullptr;     // packed weights / biases / affine params
  float* ttable = nullptr;   // [T][tb_total]
  mmd::UnetPack w;
};

namespace mmd {

static size_t push(std::vector<float>& blob, const float* p, int64_t n) {
  while (blob.size() % 4) blob.push_back(0.f);
  size_t off = blob.size();
  blob.insert(blob.end(), p, p + n);
  while (blob.size() % 4) blob.push_back(0.f);
  return off;
}
// 1 / (scale * in_scale) per channel (powers of two: exact)
static std::vector<float> inverse_scales(const std::vector<float>& sc, float in_scale = 1.f) {
  std::vector<float> r(sc.size());
  for (size_t i = 0; i < sc.size(); ++i) r[i] = 1.f / (sc[i] * in_scale);
  return r;
}
// One table of parameter records as the kernels read them (unet_kernel.h, rec_load): per unit of `cpr` adjacent channels the fields in
// order, each field's channels side by side, zero padded to whole float4; the table starts 16-byte aligned.  fields[f]: [channels]
// floats OUTSIDE the blob (it grows here).  The table is entered in the pack's directory under `name`.
static size_t push_records(std::vector<float>& blob, UnetPack& p, const std::string& name, int kind, int channels, int cpr,
                           const std::vector<const float*>& fields) {
  while (blob.size() % 4) blob.push_back(0.f);
  const size_t off = blob.size();
  const int nf = (int)fields.size(), rf = (nf * cpr + 3) / 4 * 4;
  blob.resize(off + (size_t)(channels / cpr) * rf, 0.f);
  for (int c = 0; c < channels; ++c)
    for (int f = 0; f < nf; ++f) blob[off + (size_t)(c / cpr) * rf + f * cpr + c % cpr] = fields[f][c];
  if (p.n_tables < (int)(sizeof(p.tables) / sizeof(p.tables[0]))) {
    mmd_unet_record_table& t = p.tables[p.n_tables];
    t = mmd_unet_record_table{};
    snprintf(t.name, sizeof(t.name), "%s", name.c_str());
    t.offset = off; t.kind = kind; t.channels = channels;
    t.channels_per_record = cpr; t.n_fields = nf; t.record_floats = rf;
  }
  ++p.n_tables;
  return off;
}

// The pack each of the twelve residual blocks gets (state_dict order).  pairs: interleaved column pairs, where a wave owns two
// n-tiles (every stage body but ups.0's).  Conv A's form: downs.0's first conv (4 -> 32) as one im2col chunk; the
// first block of a stage with its input whole, or as the two chunks of cat(x, skip) in the up stages; an identity block.
enum ConvAForm { A_IM2COL4, A_FIRST_WHOLE, A_FIRST_CAT, A_IDENT };
struct BlockPack { const char* name; bool pairs; ConvAForm a; };
static const BlockPack kBlockPack[12] = {
    {"d00", true, A_IM2COL4},    {"d01", true, A_IDENT},  {"d10", true, A_FIRST_WHOLE}, {"d11", true, A_IDENT},
    {"d20", true, A_FIRST_WHOLE}, {"d21", true, A_IDENT}, {"u00", false, A_FIRST_CAT},  {"u01", false, A_IDENT},
    {"u10", true, A_FIRST_CAT},  {"u11", true, A_IDENT},  {"mid1", true, A_IDENT},      {"mid2", true, A_IDENT}};

// (Spec of the fused configuration, tensors, T) -> the float blob and the offsets into it.  No HIP call: every conv gets the one
// f16x2 pack its stage body reads -- direct packs (pack_rd), the 1x1 residual conv of a stage's first RTB as a one-tap pack of its own.
static void pack_unet(const Spec& s, const float* const* tensors, int T, std::vector<float>& blob, UnetPack& p) {
  const std::vector<int> taps5 = {0, 1, 2, 3, 4}, taps3 = {0, 1, 2}, taps1 = {0};
  p.n_tables = 0;
  for (int i = 0; i < 4; ++i) p.raw_time[i] = push(blob, tensors[s.t_time[i]], s.numel[s.t_time[i]]);
  int tb_off = 0;
  const std::vector<std::vector<float>> tbmax = time_bias_absmax(tensors, s, T);
  for (int r = 0; r < 12; ++r) {
    const Rtb& R = s.rtb[r];
    const BlockPack& B = kBlockPack[r];
    RtbW& W = p.rtb[r];
    W = RtbW{};
    while (blob.size() % 4) blob.push_back(0.f);
    const int cpr = B.pairs ? 2 : 1;   // channels per record: the lane's adjacent pair, or ups.0's one channel per lane
    {                         // conv A: direct f16x2 (rd_taps) with a dynamic input scale
      const std::vector<float> sc = rd_col_scales(tensors[R.t_w0], R.cout, R.cin, 5, taps5, false), isc = inverse_scales(sc);
      if (B.a == A_IDENT) {
        W.a.wbf = pack_rd(blob, tensors[R.t_w0], R.cout, R.cin, 0, R.cin, 5, taps5, false, B.pairs, sc);
        W.a.rec = push_records(blob, p, std::string(B.name) + ".a", MMD_UNET_REC_EPI, R.cout, cpr,
                               {tensors[R.t_b0], tensors[R.t_g0], tensors[R.t_be0], isc.data()});
      } else {                // first RTB of a stage: its 1x1 residual conv [cout][cin] rides on conv A's centre tap
        const float* wres = tensors[R.t_rw];
        const std::vector<float> scr = rd_col_scales(wres, R.cout, R.cin, 1, taps1, false), iscr = inverse_scales(scr);
        W.a.rec = push_records(blob, p, std::string(B.name) + ".a", MMD_UNET_REC_EPI_RES, R.cout, cpr,
                               {tensors[R.t_b0], tensors[R.t_g0], tensors[R.t_be0], isc.data(), tensors[R.t_rb], iscr.data()});
        if (B.a == A_IM2COL4) {
          W.a.wbf = pack_im2col4(blob, tensors[R.t_w0], R.cout, false, sc);
          W.res_bf = pack_im2col4(blob, wres, R.cout, true, scr);
        } else {
          const int chunk = B.a == A_FIRST_WHOLE ? R.cin : R.cin / 2;
          W.a.wbf = pack_rd(blob, tensors[R.t_w0], R.cout, R.cin, 0, chunk, 5, taps5, false, B.pairs, sc);
          W.res_bf = pack_rd_res(blob, wres, R.cout, R.cin, 0, chunk, B.pairs, scr);
          if (B.a == A_FIRST_CAT) {
            W.a_c1_bf = pack_rd(blob, tensors[R.t_w0], R.cout, R.cin, chunk, chunk, 5, taps5, false, B.pairs, sc);
            W.res_c1_bf = pack_rd_res(blob, wres, R.cout, R.cin, chunk, chunk, B.pairs, scr);
          }
        }
      }
    }
    {                         // conv B: direct f16x2, its input scaled by the static act_a
      W.act_a = static_act_scale(tensors[R.t_g0], tensors[R.t_be0], tbmax[r], R.cout);
      const std::vector<float> sc = rd_col_scales(tensors[R.t_w1], R.cout, R.cout, 5, taps5, false), isc = inverse_scales(sc, W.act_a);
      W.b.wbf = pack_rd(blob, tensors[R.t_w1], R.cout, R.cout, 0, R.cout, 5, taps5, false, B.pairs, sc);
      W.b.rec = push_records(blob, p, std::string(B.name) + ".b", MMD_UNET_REC_EPI, R.cout, cpr,
                             {tensors[R.t_b1], tensors[R.t_g1], tensors[R.t_be1], isc.data()});
    }
    p.raw_cw[r] = push(blob, tensors[R.t_cw], (int64_t)R.cout * 32);
    p.raw_cb[r] = push(blob, tensors[R.t_cb], R.cout);
    W.tb_off = tb_off;
    tb_off += R.cout;
  }
  p.tb_total = tb_off;
  for (int i = 0; i < 2; ++i) {
    const int c = s.dims[i + 1];
    {                         // Downsample1d as a direct f16x2 conv (taps 0..2, interleaved column pairs) read at stride 2
      const std::vector<float> sct = rd_col_scales(tensors[s.t_down[i][0]], c, c, 3, taps3, false), isct = inverse_scales(sct);
      p.down[i].wbf[0] = pack_rd(blob, tensors[s.t_down[i][0]], c, c, 0, c, 3, taps3, false, true, sct);
      p.down[i].rec = push_records(blob, p, "down" + std::to_string(i), MMD_UNET_REC_TAIL_DOWN, c, 2, {tensors[s.t_down[i][1]], isct.data()});
    }
    const int cu = s.dims[2 - i];
    // ConvTranspose1d(k=4, s=2, p=1): out[2m] = in[m-1] W3 + in[m] W1 ; out[2m+1] = in[m] W2 + in[m+1] W0, as two direct f16x2
    // parity passes (ups.1: interleaved column pairs; ups.0: one channel per lane and record)
    {
      const std::vector<int> ke = {3, 1}, ko = {2, 0};
      const std::vector<float> sce = rd_col_scales(tensors[s.t_up[i][0]], cu, cu, 4, ke, true), isce = inverse_scales(sce);
      const std::vector<float> sco = rd_col_scales(tensors[s.t_up[i][0]], cu, cu, 4, ko, true), isco = inverse_scales(sco);
      p.up[i].wbf[0] = pack_rd(blob, tensors[s.t_up[i][0]], cu, cu, 0, cu, 4, ke, true, i == 1, sce);
      p.up[i].wbf[1] = pack_rd(blob, tensors[s.t_up[i][0]], cu, cu, 0, cu, 4, ko, true, i == 1, sco);
      p.up[i].rec = push_records(blob, p, "up" + std::to_string(i), MMD_UNET_REC_TAIL_UP, cu, i == 1 ? 2 : 1,
                                 {tensors[s.t_up[i][1]], isce.data(), isco.data()});
    }
  }
  {                           // final block (in ups.1's stage body): k5 conv with a dynamic input scale, 1x1 conv behind a static one
    const std::vector<float> sc = rd_col_scales(tensors[s.t_final[0]], 32, 32, 5, taps5, false), isc = inverse_scales(sc);
    p.fin.wbf = pack_rd(blob, tensors[s.t_final[0]], 32, 32, 0, 32, 5, taps5, false, true, sc);
    p.fin.rec = push_records(blob, p, "final", MMD_UNET_REC_EPI, 32, 2, {tensors[s.t_final[1]], tensors[s.t_final[2]], tensors[s.t_final[3]], isc.data()});
    p.fin_act = static_act_scale(tensors[s.t_final[2]], tensors[s.t_final[3]], std::vector<float>(32, 0.f), 32);
    std::vector<float> sc1 = rd_col_scales(tensors[s.t_final[4]], 4, 32, 1, taps1, false);
    const std::vector<float> isc1 = inverse_scales(sc1, p.fin_act);
    std::vector<float> w1(16 * 32, 0.f);      // N padded to one n-tile
    memcpy(w1.data(), tensors[s.t_final[4]], sizeof(float) * 4 * 32);
    sc1.resize(16, 1.f);
    p.fin_w1 = pack_rd(blob, w1.data(), 16, 32, 0, 32, 1, taps1, false, false, sc1);
    p.fin_rec1 = push_records(blob, p, "final.out", MMD_UNET_REC_OUT, 4, 1, {tensors[s.t_final[5]], isc1.data()});
  }
}

static int fill_time_table(const mmd_unet_s* u, const Spec& s, hipStream_t st) {
  const UnetPack& p = u->w;
  TimeArgs ta{};
  ta.w1 = u->blob + p.raw_time[0]; ta.b1 = u->blob + p.raw_time[1];
  ta.w3 = u->blob + p.raw_time[2]; ta.b3 = u->blob + p.raw_time[3];
  for (int r = 0; r < 12; ++r) {
    ta.cw[r] = u->blob + p.raw_cw[r]; ta.cb[r] = u->blob + p.raw_cb[r];
    ta.cout[r] = s.rtb[r].cout; ta.off[r] = p.rtb[r].tb_off;
  }
  ta.n_rtb = 12; ta.total = p.tb_total; ta.table = u->ttable;
  launch_time_table(ta, u->T, st);
  MMD_HIP_CHECK(hipGetLastError());
  MMD_HIP_CHECK(hipStreamSynchronize(st));
  return 0;
}

static RtbPtrs rtb_ptrs(const mmd_unet_s* u, const RtbW& w, int t) {
  RtbPtrs p{};
  p.ra = u->blob + w.a.rec; p.rb = u->blob + w.b.rec;
  p.tb = u->ttable + (size_t)t * u->w.tb_total + w.tb_off;
  p.wa_bf = w.a.wbf ? reinterpret_cast<const uint4*>(u->blob + w.a.wbf) : nullptr;
  p.wb_bf = w.b.wbf ? reinterpret_cast<const uint4*>(u->blob + w.b.wbf) : nullptr;
  p.act_a = w.act_a;
  return p;
}

// chain over RTBs rtb[0] (first) and rtb[1..n_ident] of the handle; tail = the stage's down / up conv or null
static ChainArgs args_chain(const mmd_unet_s* u, const int* rtb, int n_ident, const TailW* tail, const float* in0, int t, int n) {
  ChainArgs a{};
  a.in0 = in0; a.n = n;
  const RtbW& w0 = u->w.rtb[rtb[0]];
  a.r0 = rtb_ptrs(u, w0, t);
  a.wa0_c1_bf = w0.a_c1_bf ? reinterpret_cast<const uint4*>(u->blob + w0.a_c1_bf) : nullptr;
  a.wres_bf = w0.res_bf ? reinterpret_cast<const uint4*>(u->blob + w0.res_bf) : nullptr;
  a.wres_c1_bf = w0.res_c1_bf ? reinterpret_cast<const uint4*>(u->blob + w0.res_c1_bf) : nullptr;
  for (int k = 0; k < n_ident; ++k) a.ri[k] = rtb_ptrs(u, u->w.rtb[rtb[1 + k]], t);
  if (tail) {
    a.rt = u->blob + tail->rec;
    a.wt_bf0 = reinterpret_cast<const uint4*>(u->blob + tail->wbf[0]);
    if (tail->wbf[1]) a.wt_bf1 = reinterpret_cast<const uint4*>(u->blob + tail->wbf[1]);
  }
  return a;
}

// The kernel-argument block of a forward of n trajectories x at row t of the time table, eps = where the output goes (null: every
// step is fused, eps never leaves the workgroup).  a.fs stays disabled.
static UnetArgs unet_args(const mmd_unet_s* u, const float* x, int t, int n, float* eps) {
  // state_dict RTB indices: d00 d01 d10 d11 d20 d21 u00 u01 u10 u11 mid1 mid2 = 0..11
  static const int kD0[] = {0, 1}, kD1[] = {2, 3}, kD2[] = {4, 5, 10, 11}, kU0[] = {6, 7}, kU1[] = {8, 9};
  const UnetPack& p = u->w;
  UnetArgs a{};
  a.n = n;
  a.c[0] = args_chain(u, kD0, 1, &p.down[0], x, t, n);
  a.c[1] = args_chain(u, kD1, 1, &p.down[1], nullptr, t, n);
  a.c[2] = args_chain(u, kD2, 3, nullptr, nullptr, t, n);
  a.c[3] = args_chain(u, kU0, 1, &p.up[0], nullptr, t, n);
  a.c[4] = args_chain(u, kU1, 1, &p.up[1], nullptr, t, n);
  a.fin.out = eps;
  a.fin.w5 = reinterpret_cast<const uint4*>(u->blob + p.fin.wbf);
  a.fin.rec5 = u->blob + p.fin.rec;
  a.fin.act = p.fin_act;
  a.fin.w1_bf = reinterpret_cast<const uint4*>(u->blob + p.fin_w1);
  a.fin.rec1 = u->blob + p.fin_rec1;
  return a;
}

// The forward, with the unguided step fs fused into its tail where fs.enabled (a FusedStep{} is the plain forward).
int unet_forward_fused(mmd_unet_t u, const float* x, int t, float* eps, int n, void* ws, size_t ws_bytes, Profiler* prof,
                       hipStream_t st, const FusedStep& fs) {
  MMD_REQUIRE(u && x && eps && ws, "mmd_unet_forward: NULL argument");
  MMD_REQUIRE(n >= 1, "mmd_unet_forward: n_traj must be >= 1");
  MMD_REQUIRE(t >= 0 && t < u->T, "mmd_unet_forward: t=%d outside [0,%d)", t, u->T);
  MMD_REQUIRE(ws_bytes >= mmd_unet_workspace_bytes(u, n), "mmd_unet_forward: workspace too small");
  if (u->layered) {
    MMD_REQUIRE(!fs.enabled, "mmd_unet_forward: the fused unguided step exists in the fused kernel only");
    const bool bracket = prof_begin(prof, 0, MMD_PROF_UNET, st);
    const int rc = layered_forward(u->layered, x, t, eps, n, ws, ws_bytes, st);
    if (bracket) prof_end(prof, st);
    return rc;
  }
  UnetArgs a = unet_args(u, x, t, n, eps);
  a.fs = fs;
  const bool bracket = prof_begin(prof, 0, fs.enabled ? MMD_PROF_UNET_FUSED : MMD_PROF_UNET, st);
  // two trajectories per workgroup while that still leaves at most one workgroup per CU (256 CUs): see unet_kernel
  int rc = 0;
  if (u->precision == MMD_UNET_PRECISION_F16) {
    const int ns = n <= u->ns1_max && n <= u->ns2_max ? 1 : n <= u->ns2_max ? 2 : 4;
    rc = launch_unet_f16(ns, (n + ns - 1) / ns, st, &a, sizeof(a));
  } else if (n <= u->ns1_max && n <= u->ns2_max) hipLaunchKernelGGL(unet_kernel<1>, dim3(n), dim3(256), 0, st, a);
  else if (n <= u->ns2_max) hipLaunchKernelGGL(unet_kernel<2>, dim3((n + 1) / 2), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(unet_kernel<4>, dim3((n + 3) / 4), dim3(256), 0, st, a);
  if (bracket) prof_end(prof, st);
  if (rc) return rc;
  MMD_HIP_CHECK(hipGetLastError());
  return 0;
}

// A run of n_steps <= PERSIST_MAX_STEPS unguided steps of ALL n trajectories in one launch (unet_persist_kernel).  steps: host array of
// the steps' complete fused-step descriptors (x, hard, seed, traj0 = 0, the step's own coefficients / draw / noise and chain rows /
// t_row), copied into the workspace's table region in stream order (pageable source: staged by the runtime before the call returns).
int unet_persist_steps(mmd_unet_t u, int n, void* ws, size_t ws_bytes, hipStream_t st, const FusedStep* steps, int n_steps) {
  MMD_REQUIRE(u && !u->layered && ws && n >= 1, "unet_persist_steps: bad arguments");
  MMD_REQUIRE(n_steps >= 1 && n_steps <= PERSIST_MAX_STEPS && ws_bytes >= (size_t)PERSIST_TABLE_BYTES, "unet_persist_steps: step table");
  for (int s = 0; s < n_steps; ++s) MMD_REQUIRE(steps[s].t_row >= 0 && steps[s].t_row < u->T, "unet_persist_steps: t outside the time table");
  // (`steps` and the argument block below are PAGEABLE host memory: hipMemcpyAsync stages such a source into the runtime's own pinned
  // buffer before it returns -- the documented behaviour for pageable memory -- so the caller's stack array may be reused for the next
  // run; it also makes the copy host-synchronous, one reason this opt-in mode does not pay on the headline, and it is not legal inside a
  // stream capture, which mmd_p_sample_loop checks before it takes this path.  The first 12 KiB of the workspace are clobbered.)
  MMD_HIP_CHECK(hipMemcpyAsync(ws, steps, sizeof(FusedStep) * n_steps, hipMemcpyHostToDevice, st));
  char* const args_dev = reinterpret_cast<char*>(ws) + PERSIST_ARGS_OFF;
  // (time-table row 0: the kernel adds each step's t_row * tb_total; every step is fused, so no eps)
  const UnetArgs a = unet_args(u, reinterpret_cast<const float*>(steps[0].x), 0, n, nullptr);
  MMD_HIP_CHECK(hipMemcpyAsync(args_dev, &a, sizeof(a), hipMemcpyHostToDevice, st));   // (pageable source: staged before the call returns)
  const FusedStep* sd = reinterpret_cast<const FusedStep*>(ws);
  const UnetArgs* ap = reinterpret_cast<const UnetArgs*>(args_dev);
  if (u->precision == MMD_UNET_PRECISION_F16) {
    const int ns = n <= u->ns2_max ? 2 : 4;
    if (int rc = launch_unet_persist_f16(ns, (n + ns - 1) / ns, st, args_dev, sizeof(a), sd, n_steps, u->w.tb_total)) return rc;
  } else if (n <= u->ns2_max) hipLaunchKernelGGL(unet_persist_kernel<2>, dim3((n + 1) / 2), dim3(256), 0, st, ap, sd, n_steps, u->w.tb_total);
  else hipLaunchKernelGGL(unet_persist_kernel<4>, dim3((n + 3) / 4), dim3(256), 0, st, ap, sd, n_steps, u->w.tb_total);
  MMD_HIP_CHECK(hipGetLastError());
  return 0;
}
bool unet_fused_step_supported(mmd_unet_t u) { return u && !u->layered; }

// algorithmic FLOPs per trajectory of one forward: sum over its convs of 2 * C_out * taps * C_in * L_out
static constexpr double rtb_flops(double cin, double cout, double L) {
  return 2.0 * cout * 5 * cin * L + 2.0 * cout * 5 * cout * L + (cin != cout ? 2.0 * cout * cin * L : 0.0);
}
static const double kUnetFlops =
    rtb_flops(4, 32, 64) + rtb_flops(32, 32, 64) + 2.0 * 32 * 3 * 32 * 32 +
    rtb_flops(32, 64, 32) + rtb_flops(64, 64, 32) + 2.0 * 64 * 3 * 64 * 16 +
    rtb_flops(64, 128, 16) + 3 * rtb_flops(128, 128, 16) +
    rtb_flops(256, 64, 16) + rtb_flops(64, 64, 16) + 2.0 * 64 * 4 * 64 * 16 +
    rtb_flops(128, 32, 32) + rtb_flops(32, 32, 32) + 2.0 * 32 * 4 * 32 * 32 +
    2.0 * 32 * 5 * 32 * 64 + 2.0 * 4 * 32 * 64;

static constexpr double d5(double cin, double cout, double L) { return 2.0 * cout * 5 * cin * L; }
static const double kF16Flops =
    2 * (2.0 * 32 * 32 * 64) + 3 * d5(32, 32, 64) + 2.0 * 32 * 3 * 32 * 32 +                          // downs.0
    d5(32, 64, 32) + 2.0 * 64 * 32 * 32 + 3 * d5(64, 64, 32) + 2.0 * 64 * 3 * 64 * 16 +               // downs.1
    d5(64, 128, 16) + 2.0 * 128 * 64 * 16 + 7 * d5(128, 128, 16) +                                    // downs.2 + mid
    d5(256, 64, 16) + 2.0 * 64 * 256 * 16 + 3 * d5(64, 64, 16) + 2.0 * 64 * 4 * 64 * 16 +             // ups.0
    d5(128, 32, 32) + 2.0 * 32 * 128 * 32 + 3 * d5(32, 32, 32) + 2.0 * 32 * 4 * 32 * 32 +             // ups.1
    d5(32, 32, 64) + 2.0 * 16 * 32 * 64;                                                              // final block
static const double kFp32Flops = 0.0;                                                                 // (no fp32 MFMA left)
static const double kUnetMfmaFlops = kF16Flops + kFp32Flops;
}  // namespace mmd

extern "C" {

int mmd_unet_num_tensors(int unet_input_dim, int n_levels) {
  Spec s;
  if (!build_spec(unet_input_dim, n_levels, s)) {
    set_error("unsupported TemporalUnet configuration (unet_input_dim=%d, n_levels=%d)", unet_input_dim, n_levels);
    return -1;
  }
  return (int)s.numel.size();
}

int64_t mmd_unet_tensor_numel(int unet_input_dim, int n_levels, int index) {
  Spec s;
  if (!build_spec(unet_input_dim, n_levels, s) || index < 0 || index >= (int)s.numel.size()) return -1;
  return s.numel[index];
}

int mmd_unet_create(mmd_unet_t* out, int unet_input_dim, int n_levels, int n_diffusion_steps,
                    const float* const* tensors, const int64_t* numels, int n_tensors, const mmd_unet_options* options,
                    void* stream) {
  Spec s;
  MMD_REQUIRE(out != nullptr, "mmd_unet_create: out is NULL");
  MMD_REQUIRE(build_spec(unet_input_dim, n_levels, s),
              "unsupported TemporalUnet configuration (unet_input_dim=%d, n_levels=%d)", unet_input_dim, n_levels);
  MMD_REQUIRE(n_tensors == (int)s.numel.size(), "expected %d parameter tensors, got %d", (int)s.numel.size(), n_tensors);
  for (int i = 0; i < n_tensors; ++i)
    MMD_REQUIRE(numels[i] == s.numel[i] && tensors[i] != nullptr, "parameter tensor %d has %lld elements, expected %lld",
                i, (long long)numels[i], (long long)s.numel[i]);
  MMD_REQUIRE(n_diffusion_steps >= 1, "n_diffusion_steps must be >= 1");
  const int precision = options ? options->precision : MMD_UNET_PRECISION_F32;
  const bool layered_path = !fused_config(unet_input_dim, n_levels) || (options && (options->flags & MMD_UNET_LAYERED));
  MMD_REQUIRE(precision == MMD_UNET_PRECISION_F32 || precision == MMD_UNET_PRECISION_F16,
              "mmd_unet_options.precision = %d: MMD_UNET_PRECISION_F32 (0) or MMD_UNET_PRECISION_F16 (1)", precision);
  MMD_REQUIRE(precision == MMD_UNET_PRECISION_F32 || !layered_path,
              "mmd_unet_options.precision = MMD_UNET_PRECISION_F16 exists in the fused kernel only (unet_input_dim 32, 3 levels, "
              "without MMD_UNET_LAYERED): unet_input_dim=%d, n_levels=%d, flags=%u", unet_input_dim, n_levels, options->flags);
  hipStream_t st = (hipStream_t)stream;

  // owned until *out takes it: every early return below destroys the handle and what it has allocated by then
  struct Destroy { void operator()(mmd_unet_s* p) const { (void)mmd_unet_destroy(p); } };
  std::unique_ptr<mmd_unet_s, Destroy> u(new mmd_unet_s());
  u->T = n_diffusion_steps;
  u->precision = precision;
  if (options && options->two_per_workgroup_max != 0) u->ns2_max = options->two_per_workgroup_max < 0 ? 0 : options->two_per_workgroup_max;
  // MMD_UNET_LAYERED: the layer-by-layer path for the fused kernel's own configuration too -- the two implementations share no
  // device code, tests/test_gpu_dim_mults.py holds one against the other
  if (layered_path) {
    // e.g. UNET_DIM_MULTS[1] = (1, 2, 4, 8): layer by layer (unet_layers.hip)
    if (int rc = layered_create(&u->layered, s, n_diffusion_steps, tensors, options, st)) return rc;
  } else {
    std::vector<float> blob;
    pack_unet(s, tensors, n_diffusion_steps, blob, u->w);
    if (hipMalloc(&u->blob, blob.size() * sizeof(float)) != hipSuccess ||
        hipMalloc(&u->ttable, (size_t)u->T * u->w.tb_total * sizeof(float)) != hipSuccess) {
      set_error("mmd_unet_create: hipMalloc failed");
      return 1;
    }
    MMD_HIP_CHECK(hipMemcpyAsync(u->blob, blob.data(), blob.size() * sizeof(float), hipMemcpyHostToDevice, st));
    MMD_HIP_CHECK(hipStreamSynchronize(st));   // blob is a local vector
    u->blob_bytes = blob.size() * sizeof(float);
    if (int rc = fill_time_table(u.get(), s, st)) return rc;
  }
  *out = u.release();
  return 0;
}

int mmd_unet_destroy(mmd_unet_t u) {
  if (!u) return 0;
  layered_destroy(u->layered);
  if (u->blob) (void)hipFree(u->blob);
  if (u->ttable) (void)hipFree(u->ttable);
  delete u;
  return 0;
}

// The forward keeps every intermediate in LDS / registers; the workspace argument is kept in the ABI (callers pass the
// buffer they sized with this function) but only a token size is asked for.
size_t mmd_unet_workspace_bytes(mmd_unet_t u, int n_traj) {
  if (u && u->layered) return layered_workspace_bytes(u->layered, n_traj);   // (that path keeps its activations in the workspace)
  return n_traj > 0 ? PERSIST_TABLE_BYTES : 0;                                // (the step table of a persistent run of unguided steps)
}

int mmd_unet_forward(mmd_unet_t u, const float* x, int t, float* eps, int n, void* ws, size_t ws_bytes, void* stream) {
  return unet_forward_fused(u, x, t, eps, n, ws, ws_bytes, nullptr, (hipStream_t)stream, FusedStep{});
}

#ifdef MMD_TRACE
int mmd_debug_set_trace(void* dev_ptr) {
  return hipMemcpyToSymbol(HIP_SYMBOL(g_trace), &dev_ptr, sizeof(dev_ptr)) == hipSuccess ? 0 : 1;
}
#endif

int mmd_unet_precision(mmd_unet_t u) { return u ? u->precision : -1; }

int mmd_debug_unet_pack(int unet_input_dim, int n_levels, int n_diffusion_steps, const float* const* tensors, const int64_t* numels,
                        int n_tensors, float* blob_out, size_t blob_cap, size_t* blob_floats, mmd_unet_record_table* tables,
                        int tables_cap, int* n_tables) {
  Spec s;
  MMD_REQUIRE(fused_config(unet_input_dim, n_levels) && build_spec(unet_input_dim, n_levels, s),
              "mmd_debug_unet_pack: the fused kernel's configuration only (unet_input_dim 32, 3 levels), got (%d, %d)", unet_input_dim, n_levels);
  MMD_REQUIRE(tensors && numels && n_tensors == (int)s.numel.size(), "mmd_debug_unet_pack: expected %d parameter tensors", (int)s.numel.size());
  for (int i = 0; i < n_tensors; ++i)
    MMD_REQUIRE(numels[i] == s.numel[i] && tensors[i] != nullptr, "parameter tensor %d has %lld elements, expected %lld",
                i, (long long)numels[i], (long long)s.numel[i]);
  MMD_REQUIRE(n_diffusion_steps >= 1, "n_diffusion_steps must be >= 1");
  std::vector<float> blob;
  std::unique_ptr<UnetPack> p(new UnetPack());
  pack_unet(s, tensors, n_diffusion_steps, blob, *p);
  MMD_REQUIRE(p->n_tables <= (int)(sizeof(p->tables) / sizeof(p->tables[0])), "mmd_debug_unet_pack: %d record tables exceed the directory", p->n_tables);
  if (blob_floats) *blob_floats = blob.size();
  if (n_tables) *n_tables = p->n_tables;
  if (blob_out) memcpy(blob_out, blob.data(), sizeof(float) * (blob.size() < blob_cap ? blob.size() : blob_cap));
  if (tables)
    for (int i = 0; i < p->n_tables && i < tables_cap; ++i) tables[i] = p->tables[i];
  return 0;
}

size_t mmd_unet_weight_bytes(mmd_unet_t u) {
  if (!u) return 0;
  return u->layered ? layered_weight_bytes(u->layered) : u->blob_bytes;
}

double mmd_unet_flops_per_trajectory(void) { return kUnetFlops; }
double mmd_unet_mfma_flops_per_trajectory(void) { return kUnetMfmaFlops; }
double mmd_unet_f16x2_flops_per_trajectory(void) { return kF16Flops; }

}  // extern "C"
