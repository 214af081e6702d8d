// TemporalUnet forward, layer by layer: the host side.  For the configurations the fused kernel (unet_kernel.h) is not instantiated for --
// first of all UNET_DIM_MULTS[1] = (1, 2, 4, 8) (mmd/models/diffusion_models/temporal_unet.py:17-20, selected by a checkpoint's args.yaml at
// mmd/planners/single_agent/mpd.py:158; the released checkpoints use option 0 and run the fused kernel) -- and for MMD_UNET_LAYERED.
// One launch per layer (39 per forward of a four-level network), activations in a caller-provided HBM workspace.
//
//   ResidualTemporalBlock (layers.py:323-358): out = Mish(GN(conv5(Mish(GN(conv5(x))) + time bias))) + res(x)
//   Downsample1d = Conv1d(k3, s2, p1), Upsample1d = ConvTranspose1d(k4, s2, p1) (layers.py:261-279)
//   final_conv = Conv1dBlock(k5) + Conv1d(k1) (temporal_unet.py:104-110)
//
// Kernels: mconv_kernel (mconv_dev.h) on the matrix pipe, activations blocked [n][C / 8][L][8] -- the default: every network all of
// whose layers have whole 16-column n-tiles and GroupNorm groups (unet_input_dim 16 / 32 / 48 / 64); conv5_block_kernel and
// conv_plain_kernel (layers_valu_dev.h) on the vector ALUs, activations [n][C][L] -- the other widths, MMD_UNET_LAYERED_VALU, and the
// final 1x1 conv to eps of every network.  A model is on one or the other as a whole (LayeredUnet::mfma).
// Here: the weight packers and one record per conv (LConv); layered_create, which walks the Spec ONCE into a table of launches (LOp:
// conv, input / output / addend buffers as workspace slots, geometry); one launch-shape function per kernel family (a pure function of
// the layer's geometry, the batch size and the model's options); the kernel arguments filled by name; layered_forward, a loop over
// the table.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <map>
#include <memory>
#include <mutex>
#include <vector>

#include "common.h"
#include "f16x2.h"
#include "layers_valu_dev.h"
#include "mconv_dev.h"
#include "unet_spec.h"

namespace mmd {

namespace {

struct MPack { size_t w = 0, isc = 0; int n_chunks = 0, kch = 0; unsigned stride = 0; };   // f16x2 packs of a conv in the blob (w = 0: none)
// one conv in the blob: the vector-ALU kernels' weights [k][c_in][c_out], bias, GroupNorm affine (a Conv1dBlock's), the matrix pipe's packs
struct LConv { size_t w = 0, b = 0, g = 0, be = 0; MPack m; };
// a launch of the layer table: 0 .. 4 are mconv_kernel's KIND
enum OpKind { OP_BLOCK = 0, OP_K1 = 1, OP_DOWN = 2, OP_UP = 3, OP_RTB = 4, OP_EPS = 5 };   // Conv1dBlock, k1, k3 s2, transposed k4 s2, fused block, k1 -> eps
struct LRtb { int cin, cout; bool res; int tb_off; LConv a, b, r; };   // the two Conv1dBlocks, the 1x1 residual conv (res)
// buffers of one forward.  The first 6 + (n_levels - 1) are the workspace's, each n x 64 x unet_input_dim floats (L x C is the same at
// every level): two level inputs, the hidden tensor of a block, the output of a level's first block, a 1x1 residual, level 0's output,
// skip[j] = the output of down level j + 1; the concatenated up-path input is read from its two tensors in place
enum Slot { S_NONE = -1, S_IN0, S_IN1, S_TMP, S_MID, S_RES, S_OUT0, S_SKIP, S_X = S_SKIP + MAX_LEVELS - 1, S_EPS, N_SLOTS };
// one launch: y = conv(x1 | x2) [+ norm + Mish] + time bias + add_t
struct LOp {
  int kind = OP_BLOCK;
  const LConv* cv = nullptr, * cv2 = nullptr;   // (OP_RTB: the block's first Conv1dBlock, cv2 its second)
  int x1, x2;                         // input [n][c1][l_in] (+ [n][c2][l_in] concatenated behind it along the channels, or S_NONE)
  int y = S_NONE, add_t = S_NONE;     // output [n][c_out][l_out]; the residual added after Mish
  int tb_off = -1;                    // the block's time bias in a row of the time table, added after (the first) Mish; -1: none
  int c1, c2, c_out = 0, l_in, l_out;
  bool in_cl, out_cl = false;         // the input / output is channels-last [n][L][4] (the trajectory, eps)
  LOp(int x1_, int c1_, int L, int x2_ = S_NONE, int c2_ = 0) : x1(x1_), x2(x2_), c1(c1_), c2(c2_), l_in(L), l_out(L), in_cl(x1_ == S_X) {}
};
struct Launch { const void* fn; dim3 grid, block; size_t shm; int cs; };   // cs: output channels (GEMM columns) per blockIdx.y

}  // namespace

struct LayeredUnet {
  Spec spec;
  int T = 0, tb_total = 0;
  float* blob = nullptr;
  size_t blob_bytes = 0;
  float* ttable = nullptr;
  std::vector<LRtb> rtb;
  LConv down[MAX_LEVELS - 1], up[MAX_LEVELS - 1], fin5, fin1;
  std::vector<LOp> ops;               // the forward: built once by build_ops
  int rtb_fused = 64;                 // mmd_unet_options.rtb_fused (A/B): the widest ResidualTemporalBlock that runs as ONE launch
                                      // (0: none -- two Conv1dBlock launches each; default 64: with 128 channels the one-launch form spills)
  int mconv_max_cs = 128;             // mmd_unet_options.mconv_max_cs (A/B): the widest column slice mconv_kernel is launched with
  bool mfma = false;                  // every layer has f16x2 packs: the matrix-pipe kernels with blocked activations; else the vector-ALU kernels
  int per_sample = 0;                 // floats of the largest activation tensor of a sample (64 x unet_input_dim)
};

namespace {

// weight [c_out][c_in][k] (Conv1d) or [c_in][c_out][k] (ConvTranspose1d) -> [k][c_in][c_out]
size_t push_wt(std::vector<float>& blob, const float* w, int cout, int cin, int k, bool transposed) {
  const size_t off = blob.size();
  blob.resize(off + (size_t)k * cin * cout);
  for (int kk = 0; kk < k; ++kk)
    for (int ci = 0; ci < cin; ++ci)
      for (int co = 0; co < cout; ++co)
        blob[off + ((size_t)kk * cin + ci) * cout + co] =
            transposed ? w[((size_t)ci * cout + co) * k + kk] : w[((size_t)co * cin + ci) * k + kk];
  return off;
}
// smallest slice of a Conv1dBlock on the matrix pipe: 16, 32 or 64 output channels = whole 16-column n-tiles AND whole GroupNorm groups
// (0: none fits -- unet_input_dim 8's first level, the 24 / 40 / 56 ladders: those blocks stay on conv5_block_kernel)
int mfma_slice(int c_out) {
  if (c_out % 16) return 0;
  const int cpg = c_out / N_GROUPS;
  for (int cs : {16, 32, 64})
    if (c_out % cs == 0 && cs % cpg == 0) return cs;
  return 0;
}
// f16x2 packs of a conv given as wk [cols][cin][K] (K taps in slab-row order), one per chunk of kch input channels: kch = the input
// channels rounded up to whole K chunks of 32, at most MCONV_KCH (the k1 conv: always MCONV_KCH, its four steps are the weight ring);
// the last chunk zero-padded
MPack push_mfma(std::vector<float>& blob, const float* wk, int cols, int cin, int K) {
  MPack p{};
  const int kch = K == 1 ? MCONV_KCH : std::min(MCONV_KCH, (cin + 31) / 32 * 32);
  const int n_chunks = (cin + kch - 1) / kch;
  if (cols % 16 || n_chunks > MCONV_MAX_CHUNKS) return p;
  const int cp = K == 1 ? n_chunks * kch : (cin + 31) / 32 * 32;
  std::vector<float> wp((size_t)cols * cp * K, 0.f);
  for (int co = 0; co < cols; ++co)
    for (int ci = 0; ci < cin; ++ci)
      for (int k = 0; k < K; ++k) wp[((size_t)co * cp + ci) * K + k] = wk[((size_t)co * cin + ci) * K + k];
  std::vector<int> taps(K);
  for (int k = 0; k < K; ++k) taps[k] = k;
  const std::vector<float> sc = rd_col_scales(wp.data(), cols, cp, K, taps, false);
  p.isc = push_inverse(blob, sc);
  p.n_chunks = n_chunks;
  p.kch = kch;
  for (int j = 0; j < n_chunks; ++j) {
    const int c_lo = j * kch, cc = std::min(kch, cp - c_lo);
    const size_t o = pack_rd(blob, wp.data(), cols, cp, c_lo, cc, K, taps, false, false, sc);
    if (j == 0) p.w = o;
    if (j == 1) p.stride = (unsigned)((o - p.w) / 4);      // in 16-byte units; every chunk but the last has the same size
    if (j > 1 && (o - p.w) / 4 != (size_t)j * p.stride) return MPack{};
  }
  return p;
}
// ConvTranspose1d(k4, s2, p1) [cin][cout][4] as a k3 conv with columns 2 co + parity over rows (m - 1, m, m + 1):
// out[2 m] = in[m - 1] W3 + in[m] W1, out[2 m + 1] = in[m] W2 + in[m + 1] W0
MPack push_mfma_up(std::vector<float>& blob, const float* w, int cout, int cin) {
  std::vector<float> wk((size_t)2 * cout * cin * 3, 0.f);
  for (int co = 0; co < cout; ++co)
    for (int ci = 0; ci < cin; ++ci) {
      const float* k = w + ((size_t)ci * cout + co) * 4;
      float* e = wk.data() + ((size_t)(2 * co) * cin + ci) * 3;
      float* o = wk.data() + ((size_t)(2 * co + 1) * cin + ci) * 3;
      e[0] = k[3]; e[1] = k[1];
      o[1] = k[2]; o[2] = k[0];
    }
  return push_mfma(blob, wk.data(), 2 * cout, cin, 3);
}
size_t push_v(std::vector<float>& blob, const float* p, int64_t n) {
  const size_t off = blob.size();
  blob.insert(blob.end(), p, p + n);
  return off;
}
// a conv of `kind` (OP_BLOCK .. OP_UP) into its record: P_VALU = weights, bias and (g given) GroupNorm affine for the vector-ALU kernels,
// P_PACK = the f16x2 packs (a Conv1dBlock's only where its slice is whole GroupNorm groups).  Two calls where the blob's order has other
// tensors between the two parts: the packs are read as uint4, so their alignment follows from everything pushed before them
enum { P_VALU = 1, P_PACK = 2, P_BOTH = 3 };
void push_conv(std::vector<float>& blob, LConv& c, int parts, int kind, int cout, int cin, const float* w, const float* b = nullptr,
               const float* g = nullptr, const float* be = nullptr) {
  if (parts & P_VALU) {
    c.w = push_wt(blob, w, cout, cin, kind == OP_BLOCK ? 5 : kind == OP_K1 ? 1 : kind == OP_DOWN ? 3 : 4, kind == OP_UP);
    c.b = push_v(blob, b, cout);
    if (g) c.g = push_v(blob, g, cout), c.be = push_v(blob, be, cout);
  }
  if (!(parts & P_PACK)) return;
  if (kind == OP_BLOCK) c.m = mfma_slice(cout) ? push_mfma(blob, w, cout, cin, 5) : MPack{};
  else c.m = kind == OP_UP ? push_mfma_up(blob, w, cout, cin) : push_mfma(blob, w, cout, cin, kind == OP_K1 ? 1 : 3);
}
// the network as a list of launches (temporal_unet.py:147-175); u->rtb / down / up / fin* are final: the ops point into them
void build_ops(LayeredUnet* u) {
  const Spec& s = u->spec;
  const int NL = s.n_levels;
  auto conv = [&](LOp o, int kind, const LConv& cv, int c_out, int y) -> LOp& {
    o.kind = kind; o.cv = &cv; o.c_out = c_out; o.y = y;
    u->ops.push_back(o);
    return u->ops.back();
  };
  // one ResidualTemporalBlock (layers.py:346-358): in -> out [cout][L].  Matrix pipe, 32 / 64 / 128 output channels: the two Conv1dBlocks in
  // ONE launch (mconv_kernel KIND 4: the hidden tensor stays in the workgroup; same bits as the two launches)
  auto rtb = [&](const LRtb& R, const LOp& in, int out) {
    const bool fused = u->mfma && R.b.m.n_chunks == 1 && (R.cout == 32 || R.cout == 64 || R.cout == 128) && R.cout <= u->rtb_fused;
    const int res = R.res ? S_RES : in.x1;                   // identity residual (cin == cout: never a concatenated input)
    if (fused && R.res) conv(in, OP_K1, R.r, R.cout, S_RES);
    LOp& a = conv(in, fused ? OP_RTB : OP_BLOCK, R.a, R.cout, fused ? out : S_TMP);
    a.tb_off = R.tb_off;
    if (fused) { a.cv2 = &R.b; a.add_t = res; return; }
    if (R.res) conv(in, OP_K1, R.r, R.cout, S_RES);
    conv(LOp(S_TMP, R.cout, in.l_in), OP_BLOCK, R.b, R.cout, out).add_t = res;
  };
  int L = H, xin = S_X, level_out = S_OUT0;
  for (int i = 0; i < NL; ++i) {                              // downs (temporal_unet.py:147-156)
    const int c = s.dims[i + 1];
    level_out = i == 0 ? S_OUT0 : S_SKIP + i - 1;
    rtb(u->rtb[2 * i], LOp(xin, s.dims[i], L), S_MID);
    rtb(u->rtb[2 * i + 1], LOp(S_MID, c, L), level_out);
    if (i == NL - 1) break;
    xin = S_IN0 + (i & 1);
    conv(LOp(level_out, c, L), OP_DOWN, u->down[i], c, xin).l_out = L / 2;
    L /= 2;
  }
  const int m0 = 2 * NL + 2 * (NL - 1);                       // mid blocks (state_dict order: behind the ups)
  rtb(u->rtb[m0], LOp(level_out, s.dims[NL], L), S_MID);
  rtb(u->rtb[m0 + 1], LOp(S_MID, s.dims[NL], L), S_IN0);
  for (int i = 0; i < NL - 1; ++i) {                          // ups: x = cat(x, h.pop()) (temporal_unet.py:164-171)
    const int din = s.dims[NL - 1 - i], dout = s.dims[NL - i];
    rtb(u->rtb[2 * NL + 2 * i], LOp(S_IN0, dout, L, S_SKIP + NL - 2 - i, dout), S_MID);
    rtb(u->rtb[2 * NL + 2 * i + 1], LOp(S_MID, din, L), S_IN1);
    conv(LOp(S_IN1, din, L), OP_UP, u->up[i], din, S_IN0).l_out = 2 * L;
    L *= 2;
  }
  // final_conv (temporal_unet.py:104-110); with one level there are no ups and L is still 64
  conv(LOp(S_IN0, s.uid, L), OP_BLOCK, u->fin5, s.uid, S_MID);
  conv(LOp(S_MID, s.uid, L), OP_EPS, u->fin1, 4, S_EPS).out_cl = true;
}

template <int KIND, int NBH>
const void* mconv_fn(int cs) {
  return cs == 128 ? (const void*)mconv_kernel<2, 4, KIND, NBH> : cs == 64 ? (const void*)mconv_kernel<1, 4, KIND, NBH>
       : cs == 32 ? (const void*)mconv_kernel<1, 2, KIND, NBH> : (const void*)mconv_kernel<1, 1, KIND, NBH>;
}
template <int KIND>
const void* mconv_fn(int cs, int kch) { return kch <= 64 ? mconv_fn<KIND, 1>(cs) : mconv_fn<KIND, 2>(cs); }
constexpr int kNumCUs = 256;                       // MI355X
// workgroups of `fn` with `shm` bytes of LDS that one CU holds (cached: the launches of a forward ask 47 times)
int mconv_resident(const void* fn, size_t shm) {
  static std::mutex mu;
  static std::map<std::pair<const void*, size_t>, int> cache;
  std::lock_guard<std::mutex> lock(mu);
  auto it = cache.find({fn, shm});
  if (it != cache.end()) return it->second;
  int nb = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fn, 256, shm) != hipSuccess || nb < 1) nb = 1;
  cache[{fn, shm}] = nb;
  return nb;
}
template <int KIND>
int mconv_set_lds() {
  for (int cs : {16, 32, 64, 128})
    for (int kch : {64, 128}) MMD_HIP_CHECK(hipFuncSetAttribute(mconv_fn<KIND>(cs, kch), hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024));
  return 0;
}

// ---- the launch shape of an op at batch size n, one function per kernel family.  (The compiler lays the kernels out in the order in
// which this file first names them -- conv5_block_kernel<1>, <2>, <4>, then mconv_kernel by KIND, then conv_plain_kernel: keep it.  With
// mconv_kernel named first, the same kernels in another order, a forward took 1.0 - 1.7 us (0.1 - 0.4 %) longer:
// profiles/layered_single_source_ab.txt)
// conv5_block_kernel: a workgroup of KS x nt threads, nt from the slice's nconv = (L / 4) * (cs / CT) register tiles, aimed at [16, 64]:
// the slice width cs (whole GroupNorm groups) follows from that, CT = 2 / 4 for the big launches
int conv5_shape(const LOp& op, int n, Launch& l) {
  const int L = op.l_in, c_out = op.c_out, cpg = c_out / N_GROUPS;
  int ct = n >= 768 ? 4 : n >= 192 ? 2 : 1, cs = c_out;
  auto nconv = [&]() { return (L / 4) * (cs / ct); };
  while (nconv() > 64 && (cs / 2) % cpg == 0) cs /= 2;
  while (ct > 1 && (cs % ct || nconv() < 16)) ct /= 2;
  // threads per partial sum: the slice's register tiles, in whole quarter-waves, at most 64 -- a thread loops over more (a group
  // of 5 or 7 channels, or one group of 512 outputs at unet_input_dim 64, does not cut into 16 .. 64 tiles)
  const int nt = nconv() >= 64 ? 64 : (nconv() + 15) / 16 * 16;
  MMD_REQUIRE((ct == 1 || ct == 2 || ct == 4) && cs % ct == 0 && cs % cpg == 0 && c_out % cs == 0 && (KS * nt) % 64 == 0 && KS * nt <= 256,
              "layered_forward: no launch shape for a Conv1dBlock of %d channels at length %d", c_out, L);
  l.fn = ct == 1 ? (const void*)conv5_block_kernel<1> : ct == 2 ? (const void*)conv5_block_kernel<2> : (const void*)conv5_block_kernel<4>;
  l.grid = dim3(n, c_out / cs); l.block = dim3(KS * nt); l.cs = cs;
  l.shm = ((size_t)(op.c1 + op.c2) * (L + 8) + (size_t)KS * cs * L + 2 * N_GROUPS) * sizeof(float);
  return 0;
}
// mconv_kernel: a workgroup = 64 / (rows of a sample) samples x a slice of <= 128 of the GEMM's columns; narrower slices (down to whole
// n-tiles, for a Conv1dBlock whole GroupNorm groups) while the launch has fewer than 3 workgroups per CU
int mconv_shape(const LayeredUnet* u, const LOp& op, int n, Launch& l) {
  const int kind = op.kind, cols = kind == OP_UP ? 2 * op.c_out : op.c_out;
  const int unit = kind == OP_BLOCK ? mfma_slice(op.c_out) : kind == OP_RTB ? cols : 16;
  const MPack& mp = op.cv->m;
  const int rows = kind == OP_DOWN ? op.l_in / 2 : op.l_in, spw = 64 / rows, n_wg = (n + spw - 1) / spw;
  int cs = 0;                                              // the widest slice that leaves >= 768 workgroups, else the narrowest there is
  for (int w : {128, 64, 32, 16})
    if (w <= u->mconv_max_cs && cols % w == 0 && w % unit == 0 && (!cs || (long long)n_wg * (cols / cs) < 768)) cs = w;
  if (kind == OP_RTB) cs = cols;                           // a whole ResidualTemporalBlock: one slice (32, 64 or 128 channels)
  MMD_REQUIRE(cs && rows >= 8 && rows <= 64, "layered_forward: no slice for a layer of %d columns", cols);
  if (kind == OP_RTB)
    MMD_REQUIRE(op.cv2 && op.cv2->m.w && op.cv2->m.n_chunks == 1 && (cols == 32 || cols == 64 || cols == 128), "layered_forward: no fused block of %d channels", cols);
  // LDS: the widest slab (the staged chunk; KIND 4: also the hidden tensor's c_out channels), or the output tile over it
  const size_t slab = (size_t)2 * (std::max(mp.kch, kind == OP_RTB ? cols : 0) / 8) * spw * (op.l_in + 4) * 16,
               outs = kind == OP_BLOCK || kind == OP_RTB ? (size_t)cs * OST * 4 : 0;
  l.shm = std::max(slab, outs) + (64 + 24) * sizeof(float);   // + the statistics' exchange + the samples' maxima
  l.fn = kind == 0 ? mconv_fn<0>(cs, mp.kch) : kind == 1 ? mconv_fn<1>(cs, mp.kch) : kind == 2 ? mconv_fn<2>(cs, mp.kch)
       : kind == 3 ? mconv_fn<3>(cs, mp.kch) : mconv_fn<4>(cs, mp.kch);
  // the items (64 / rows samples each) of a slice go to as many workgroups as the chip holds at once, the same number each (+- 1): a
  // workgroup requests its next item's rows under the current one's GEMM and tail
  const int ny = cols / cs, cap = std::max(1, mconv_resident(l.fn, l.shm) * kNumCUs / ny), per_wg = (n_wg + cap - 1) / cap;
  l.grid = dim3((n_wg + per_wg - 1) / per_wg, ny); l.block = dim3(256); l.cs = cs;
  return 0;
}
// conv_plain_kernel: the output channels of a launch (>= 32) split over blockIdx.y, in multiples of 8, until it has >= 3 workgroups per
// CU (or 8 slices)
int plain_shape(const LOp& op, int n, Launch& l) {
  int ns = 1;
  while (op.c_out >= 32 && ns < N_GROUPS && (long long)n * ns < 768 && (op.c_out / (2 * ns)) % 8 == 0) ns *= 2;
  l.fn = op.kind == OP_UP ? (const void*)conv_plain_kernel<1, 4, 2> : op.kind == OP_DOWN ? (const void*)conv_plain_kernel<0, 3, 2> : (const void*)conv_plain_kernel<0, 1, 1>;
  l.grid = dim3(n, ns); l.block = dim3(256); l.cs = op.c_out / ns;
  l.shm = (size_t)op.l_in * (op.c1 + op.c2) * sizeof(float);
  return 0;
}

// ---- the kernel arguments of an op, by name: buf = this call's buffers by slot, tt = its row of the time table, cs = the launch's slice;
// valu: a vector-ALU kernel, which takes m.c alone
MConvArgs layer_args(const LayeredUnet* u, const LOp& op, float* const* buf, const float* tt, int n, int cs, bool valu) {
  const float* B = u->blob;
  const bool norm = op.kind == OP_BLOCK || op.kind == OP_RTB;
  MConvArgs m{};
  ConvArgs& a = m.c;
  a.x1 = buf[op.x1]; a.x2 = op.x2 == S_NONE ? nullptr : buf[op.x2]; a.y = buf[op.y];
  a.c1 = op.c1; a.c2 = op.c2; a.c_out = op.c_out; a.cs = cs;
  a.l_in = op.l_in; a.l_out = op.l_out; a.in_cl = op.in_cl; a.out_cl = op.out_cl;
  a.wt = valu ? B + op.cv->w : nullptr; a.bias = B + op.cv->b;
  a.gamma = norm ? B + op.cv->g : nullptr; a.beta = norm ? B + op.cv->be : nullptr;
  a.add_c = op.tb_off < 0 ? nullptr : tt + op.tb_off; a.add_t = op.add_t == S_NONE ? nullptr : buf[op.add_t];
  a.in_bl = valu && u->mfma && !op.in_cl;                  // (a vector-ALU conv of a matrix-pipe model: the 1x1 conv to eps)
  if (valu) return m;
  const MPack& mp = op.cv->m;
  m.wpk = reinterpret_cast<const uint4*>(B + mp.w); m.isc = B + mp.isc;
  m.stride = mp.stride; m.n_chunks = mp.n_chunks; m.kch = mp.kch; m.n = n;
  if (op.kind == OP_RTB) {
    m.wpk2 = reinterpret_cast<const uint4*>(B + op.cv2->m.w); m.isc2 = B + op.cv2->m.isc;
    m.bias2 = B + op.cv2->b; m.gamma2 = B + op.cv2->g; m.beta2 = B + op.cv2->be;
  }
  return m;
}

}  // namespace

int layered_create(LayeredUnet** out, const Spec& s, int T, const float* const* tensors, const mmd_unet_options* opt, hipStream_t st) {
  // (owned until the last step succeeded: no error path below leaks the device allocations or the host object)
  std::unique_ptr<LayeredUnet, void (*)(LayeredUnet*)> owner(new LayeredUnet(), layered_destroy);
  LayeredUnet* u = owner.get();
  u->spec = s; u->T = T; u->per_sample = H * s.uid;
  std::vector<float> blob;
  size_t raw_time[4], raw_cw[MAX_RTB], raw_cb[MAX_RTB];
  bool packs = true;                  // every conv has f16x2 packs and whole channel blocks to read
  for (int i = 0; i < 4; ++i) raw_time[i] = push_v(blob, tensors[s.t_time[i]], s.numel[s.t_time[i]]);
  for (size_t r = 0; r < s.rtb.size(); ++r) {
    const Rtb& R = s.rtb[r];
    LRtb L{};
    L.cin = R.cin; L.cout = R.cout; L.res = R.res;
    push_conv(blob, L.a, P_VALU, OP_BLOCK, R.cout, R.cin, tensors[R.t_w0], tensors[R.t_b0], tensors[R.t_g0], tensors[R.t_be0]);
    push_conv(blob, L.b, P_VALU, OP_BLOCK, R.cout, R.cout, tensors[R.t_w1], tensors[R.t_b1], tensors[R.t_g1], tensors[R.t_be1]);
    if (R.res) push_conv(blob, L.r, P_BOTH, OP_K1, R.cout, R.cin, tensors[R.t_rw], tensors[R.t_rb]);
    push_conv(blob, L.a, P_PACK, OP_BLOCK, R.cout, R.cin, tensors[R.t_w0]);
    push_conv(blob, L.b, P_PACK, OP_BLOCK, R.cout, R.cout, tensors[R.t_w1]);
    raw_cw[r] = push_v(blob, tensors[R.t_cw], (int64_t)R.cout * 32); raw_cb[r] = push_v(blob, tensors[R.t_cb], R.cout);
    packs = packs && L.a.m.w && L.b.m.w && (!R.res || L.r.m.w) && (r == 0 || R.cin % 8 == 0);
    L.tb_off = u->tb_total; u->tb_total += R.cout;
    u->rtb.push_back(L);
  }
  for (int i = 0; i < s.n_levels - 1; ++i) {
    const int c = s.dims[i + 1], cu = s.dims[s.n_levels - 1 - i];
    push_conv(blob, u->down[i], P_BOTH, OP_DOWN, c, c, tensors[s.t_down[i][0]], tensors[s.t_down[i][1]]);
    push_conv(blob, u->up[i], P_BOTH, OP_UP, cu, cu, tensors[s.t_up[i][0]], tensors[s.t_up[i][1]]);
    packs = packs && u->down[i].m.w && u->up[i].m.w;
  }
  push_conv(blob, u->fin5, P_PACK, OP_BLOCK, s.uid, s.uid, tensors[s.t_final[0]]);
  push_conv(blob, u->fin5, P_VALU, OP_BLOCK, s.uid, s.uid, tensors[s.t_final[0]], tensors[s.t_final[1]], tensors[s.t_final[2]], tensors[s.t_final[3]]);
  push_conv(blob, u->fin1, P_VALU, OP_K1, 4, s.uid, tensors[s.t_final[4]], tensors[s.t_final[5]]);
  if (opt && opt->rtb_fused >= 0) u->rtb_fused = opt->rtb_fused;
  if (opt && opt->mconv_max_cs >= 16) u->mconv_max_cs = opt->mconv_max_cs;
  const bool valu_only = opt && (opt->flags & MMD_UNET_LAYERED_VALU);     // every layer on the vector-ALU kernels (A/B of mconv_kernel)
  u->mfma = !valu_only && packs && u->fin5.m.w && s.uid % 8 == 0;
  build_ops(u);
  if (hipMalloc(&u->blob, blob.size() * sizeof(float)) != hipSuccess ||
      hipMalloc(&u->ttable, (size_t)T * u->tb_total * sizeof(float)) != hipSuccess) {
    set_error("mmd_unet_create: hipMalloc failed");
    return 1;
  }
  // widest Conv1dBlock input: ups.0.0 of a four-level net stages 2 x 8 uid x 8 channels x (8 + 8) positions (64 KB at uid 64)
  for (const void* f : {(const void*)conv5_block_kernel<1>, (const void*)conv5_block_kernel<2>, (const void*)conv5_block_kernel<4>})
    MMD_HIP_CHECK(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024));
  if (mconv_set_lds<0>() || mconv_set_lds<1>() || mconv_set_lds<2>() || mconv_set_lds<3>() || mconv_set_lds<4>()) return 1;
  MMD_HIP_CHECK(hipMemcpyAsync(u->blob, blob.data(), blob.size() * sizeof(float), hipMemcpyHostToDevice, st));
  MMD_HIP_CHECK(hipStreamSynchronize(st));
  u->blob_bytes = blob.size() * sizeof(float);
  TimeArgs ta{};
  ta.w1 = u->blob + raw_time[0]; ta.b1 = u->blob + raw_time[1];
  ta.w3 = u->blob + raw_time[2]; ta.b3 = u->blob + raw_time[3];
  for (size_t r = 0; r < s.rtb.size(); ++r) {
    ta.cw[r] = u->blob + raw_cw[r]; ta.cb[r] = u->blob + raw_cb[r];
    ta.cout[r] = s.rtb[r].cout; ta.off[r] = u->rtb[r].tb_off;
  }
  ta.n_rtb = (int)s.rtb.size(); ta.total = u->tb_total; ta.table = u->ttable;
  launch_time_table(ta, T, st);
  MMD_HIP_CHECK(hipGetLastError());
  MMD_HIP_CHECK(hipStreamSynchronize(st));
  *out = owner.release();
  return 0;
}

void layered_destroy(LayeredUnet* u) {
  if (!u) return;
  if (u->blob) (void)hipFree(u->blob);
  if (u->ttable) (void)hipFree(u->ttable);
  delete u;
}

static int n_buffers(const LayeredUnet* u) { return S_SKIP + (u->spec.n_levels - 1); }
size_t layered_weight_bytes(const LayeredUnet* u) { return u->blob_bytes; }
size_t layered_workspace_bytes(const LayeredUnet* u, int n_traj) {
  return n_traj > 0 ? (size_t)n_buffers(u) * n_traj * u->per_sample * sizeof(float) + 256 : 0;
}

int layered_forward(const LayeredUnet* u, const float* x, int t, float* eps, int n, void* ws, size_t ws_bytes, hipStream_t st) {
  MMD_REQUIRE(ws_bytes >= layered_workspace_bytes(u, n), "mmd_unet_forward: workspace too small");
  float* buf[N_SLOTS] = {};
  for (int i = 0; i < n_buffers(u); ++i) buf[i] = reinterpret_cast<float*>(ws) + (size_t)i * n * u->per_sample;
  buf[S_X] = const_cast<float*>(x); buf[S_EPS] = eps;      // (x is read only: no op's y)
  const float* tt = u->ttable + (size_t)t * u->tb_total;
  for (const LOp& op : u->ops) {
    const bool valu = !u->mfma || op.out_cl;               // (the matrix-pipe kernel writes blocked activations only)
    Launch l{};
    MMD_REQUIRE(valu || (op.cv->m.w && (op.in_cl ? op.c1 == 4 && !op.c2 : op.c1 % 8 == 0 && op.c2 % 8 == 0)),
                "layered_forward: a %s of %d -> %d channels has no matrix-pipe form",
                op.kind == OP_BLOCK ? "Conv1dBlock" : op.kind == OP_RTB ? "block" : "conv", op.c1 + op.c2, op.c_out);
    if (int rc = !valu ? mconv_shape(u, op, n, l) : op.kind == OP_BLOCK ? conv5_shape(op, n, l) : plain_shape(op, n, l)) return rc;
    MConvArgs m = layer_args(u, op, buf, tt, n, l.cs, valu);
    MMD_REQUIRE(!m.c.in_bl || !m.c.x2, "layered_forward: a blocked input is one tensor");
    void* args[] = {valu ? (void*)&m.c : (void*)&m};
    MMD_HIP_CHECK(hipLaunchKernel(l.fn, l.grid, l.block, args, l.shm, st));
  }
  MMD_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace mmd

#ifdef MCONV_TIMING
extern "C" __attribute__((visibility("default"))) int mmd_debug_mconv_clocks(unsigned long long* out) {   // [5][4][9][8], cleared after the read
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(mmd::g_mconv_clk), sizeof(mmd::g_mconv_clk)) != hipSuccess) return 1;
  static unsigned long long zero[5 * 4 * 9 * 8];
  return hipMemcpyToSymbol(HIP_SYMBOL(mmd::g_mconv_clk), zero, sizeof(zero)) != hipSuccess;
}
#endif
