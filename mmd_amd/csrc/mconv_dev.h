// mconv_kernel: a layer of the layer-by-layer TemporalUnet on the matrix pipe (host side: unet_layers.hip).
#pragma once
#include <type_traits>

#include "f16x2.h"
#include "gn_mish.h"
#include "layers_valu_dev.h"

namespace mmd {

namespace {

// The layer-by-layer path ON THE MATRIX PIPE (round 5): fp32 arithmetic as the two-piece fp16 split of f16x2.h (three
// v_mfma_f32_16x16x32_f16 per product, fp32 accumulate -- the fused kernel's building blocks), for a network whose every layer has GEMM
// columns in whole 16-column n-tiles.  KIND 0: Conv1dBlock (conv k5 + GroupNorm + Mish + addends); 1: Conv1d k1 (the 1x1 residual); 2:
// Conv1d k3 stride 2 (Downsample1d); 3: ConvTranspose1d(k4, s2, p1) (Upsample1d) as a k3 conv with 2 c_out columns (column 2 co + parity:
// out[2 m] = in[m - 1] W3 + in[m] W1, out[2 m + 1] = in[m] W2 + in[m + 1] W0) and an interleaving store.
// ACTIVATIONS between the layers are stored BLOCKED, [n][C / 8][L][8 channels]: the 8 channels of a position are 32 contiguous bytes, so
// the staging below reads whole rows of its LDS layout (two 16-byte loads) and the epilogues write runs of channels (the trajectory in
// and eps out keep the caller's channels-last layout).
// GEMM: M = (sample, output row) -- an ITEM is SPW = 64 / LR consecutive samples (LR = rows of a sample: l_in, or l_in / 2 for the strided
// conv), so M is always 64 rows = four M tiles and a weight fragment is used on all of them, as in the fused kernel; N = a
// slice of cs in {16, 32, 64, 128} columns (blockIdx.y; whole GroupNorm groups for KIND 0); K = taps x input channels, in CHUNKS of kch <=
// 128 channels:
//   * per chunk the samples' rows go to LDS as fp16 pieces in ROW form [piece][channel block b = KCj g + kc][row = (l_in + 4) sample + 2 +
//     position][8 channels] (16 bytes per (block, row): an A fragment is one ds_read_b128; two zero rows either side of a sample are the
//     conv's padding, a tap is a row offset, the stride a row step) under a dynamic power-of-two scale PER SAMPLE AND CHUNK from the exact
//     maximum of the staged values (dyn_scale; the maximum is taken on the registers the loads land in, through LDS atomics -- no second
//     pass over the input).  The accumulators live across the chunks in units of the current chunk's scale: a new chunk multiplies them
//     by the ratio of the two scales (a power of two: exact);
//   * weights: host-packed per layer and chunk in B-fragment order [chunk][n-tile][tap][kc][piece][lane] x 16 bytes with per-column
//     power-of-two scales (pack_rd / rd_col_scales of f16x2.h), streamed from L2 through a register ring of RD steps (RD divides a chunk's
//     steps: 5 taps, 3 taps, or the k1 conv's chunk always padded to four K chunks);
//   * a wave takes NTW n-tiles x MTW M tiles (cs <= 32: the waves that share an n-tile split the M tiles);
//   * KIND 0: the accumulators go -- scaled back per channel and sample, bias added -- to an LDS tile that re-uses the slab; a thread then
//     owns 4 rows x cs / 16 adjacent channels of it in registers: the GroupNorm statistics (two passes: mean, then squared deviations) are
//     sums over those and a FIXED balanced tree over the channel index, then over the rows (lanes, then waves), so the bits do not depend
//     on the slicing; normalise + Mish + addend as the fused kernel (gn_mish.h).  The plain convs store from the accumulators.
// A launch has as many workgroups as the chip holds at once; a workgroup (4 waves) takes the items blockIdx.x, + gridDim.x, ... of its slice
// as a sequence of STAGES (item, chunk), and requests the next stage's rows right behind the current stage's conversion, so that they land
// under its GEMM and tail (the widest slice, whose registers are the weight ring's, requests them at the stage's start).
// A sample's arithmetic does not depend on the batch it sits in, on its place in the workgroup or on the slicing.
constexpr int MCONV_KCH = 128;                     // input channels staged per chunk (at most)
constexpr int MCONV_MAX_CHUNKS = 8;                // <= 1024 input channels
constexpr int OST = 68;                            // row stride of the LDS output tile [channel][64 (sample, position) rows]
struct MConvArgs {
  ConvArgs c;                         // x1 / x2 / c1 / c2 / l_in / l_out / c_out / cs (columns of the slice) / in_cl / bias / gamma / beta / add_c / add_t / y
  const uint4* wpk;                   // the layer's packs; chunk j starts at wpk + j stride: n-tiles x taps x kcj chunks x 2 pieces x 64 lanes
  const float* isc;                   // [columns] inverse weight scales
  unsigned stride;                    // (every chunk but the last is kch channels wide: one stride)
  int n_chunks, kch, n;
  // KIND 4: the block's second Conv1dBlock (c_out -> c_out, one chunk): its packs and GroupNorm parameters; c.add_c (the time bias)
  // follows the first conv, c.add_t (the residual) the second
  const uint4* wpk2;
  const float* isc2;
  const float* bias2; const float* gamma2; const float* beta2;
};
// -DMCONV_TIMING (tools/dbg/mconv_phases.py builds it): wave 0 of every workgroup adds its clock64() phase times to a table indexed by
// (KIND, log2 l_in - 3, NTW * MTW): staging loads + maxima, conversion, GEMM, exchange, statistics, tail, whole; read and cleared by
// mmd_debug_mconv_clocks
#ifdef MCONV_TIMING
__device__ unsigned long long g_mconv_clk[5][4][9][8];
#define MCONV_T(i) if (tid == 0) { const long long now_ = clock64(); clk_[i] += now_ - last_; last_ = now_; }
#else
#define MCONV_T(i)
#endif
template <int KIND> struct MKind;
template <> struct MKind<0> { static constexpr int K = 5, S = 1, RD = 5, NR = 3; };
template <> struct MKind<1> { static constexpr int K = 1, S = 1, RD = 4, NR = 3; };
template <> struct MKind<2> { static constexpr int K = 3, S = 2, RD = 3, NR = 5; };
template <> struct MKind<3> { static constexpr int K = 3, S = 1, RD = 3, NR = 3; };
template <> struct MKind<4> { static constexpr int K = 5, S = 1, RD = 5, NR = 3; };   // a whole ResidualTemporalBlock: two KIND 0 convs
// V adjacent floats (V = 1, 2, 4 or 8) of a blocked tensor from / to global memory (a run inside one 32-byte block: 4 V-byte aligned)
template <int V> __device__ __forceinline__ void ld_run(float (&d)[V], const float* p) {
  if constexpr (V == 1) d[0] = p[0];
  else if constexpr (V == 2) { const float2 q = *reinterpret_cast<const float2*>(p); d[0] = q.x; d[1] = q.y; }
  else {
#pragma unroll
    for (int j = 0; j < V; j += 4) { const float4 q = *reinterpret_cast<const float4*>(p + j); d[j] = q.x; d[j + 1] = q.y; d[j + 2] = q.z; d[j + 3] = q.w; }
  }
}
template <int V> __device__ __forceinline__ void st_run(float* p, const float (&d)[V]) {
  if constexpr (V == 1) p[0] = d[0];
  else if constexpr (V == 2) *reinterpret_cast<float2*>(p) = make_float2(d[0], d[1]);
  else {
#pragma unroll
    for (int j = 0; j < V; j += 4) *reinterpret_cast<float4*>(p + j) = make_float4(d[j], d[j + 1], d[j + 2], d[j + 3]);
  }
}
// NTW n-tiles x MTW M tiles per wave: (2, 4) for a slice of 128 columns, (1, 4) for 64, (1, 2) for 32, (1, 1) for 16 -- compile-time, so
// that the weight ring's slots are registers with exact s_waitcnt counts (with run-time tile counts the compiler drained every load)
// NBH: channel blocks per staging thread (1: chunks of <= 64 channels, three workgroups per CU; 2: up to 128)
template <int NTW, int MTW, int KIND, int NBH>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(NTW == 1 && NBH == 1 && KIND != 4 ? 3 : 2))) void mconv_kernel(MConvArgs m) {
  constexpr int K = MKind<KIND>::K, S = MKind<KIND>::S, RD = MKind<KIND>::RD, NR = MKind<KIND>::NR;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const ConvArgs& a = m.c;
  const int cin = a.c1 + a.c2, L = a.l_in, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lsh_in = 31 - __builtin_clz(L);                // l_in is 8, 16, 32 or 64
  const int lsh = lsh_in - (S - 1), LR = 1 << lsh;         // GEMM rows of a sample
  const int SPW = 64 >> lsh, RS = L + 4, SROWS = SPW * RS;  // samples per workgroup, slab rows per sample / in all
  const int c0 = blockIdx.y * a.cs, n_items = (m.n + SPW - 1) / SPW;   // an item = SPW consecutive samples; the workgroup takes items blockIdx.x, + gridDim.x, ...
#ifdef MCONV_TIMING
  long long clk_[6] = {}, last_ = clock64();
  const long long first_ = last_;
#endif
  char* const slab = smem;
  // LDS: [slab: 2 pieces x (kch / 8) blocks x SROWS x 16 B | KIND 0: the output tile [cs][OST] aliases it] [red: 4 waves x 16 partial sums]
  // [smax: 2 x 8 per-sample maxima (as uint: non-negative floats order like their bits), alternating between the stages; 8 more for the
  // hidden tensor of KIND 4]
  const int slab_ch = KIND == 4 && a.c_out > m.kch ? a.c_out : m.kch;   // (KIND 4: the hidden tensor's c_out channels are a slab too)
  const int slab_bytes = 2 * (slab_ch / 8) * SROWS * 16, outs_bytes = KIND == 0 || KIND == 4 ? a.cs * OST * 4 : 0;
  float* const red = reinterpret_cast<float*>(smem + (slab_bytes > outs_bytes ? slab_bytes : outs_bytes));
  unsigned* const smax = reinterpret_cast<unsigned*>(red + 64);
  // (the per-sample maxima, the `red` partials and the slab bookkeeping hold at most 8 samples per item: a sample has >= 8 GEMM rows --
  // H = 64 over at most MAX_LEVELS = 4 levels, the stride-2 conv never runs at the last level -- which mconv() on the host checks
  // (`rows >= 8`); a launch that breaks it must not scribble past smax)
  if (SPW > 8) __builtin_trap();
  if (tid < 24) smax[tid] = 0u;
  // ---- this thread's staging rows of an item: rows tid % 32 + 32 i of the slab -> (sample, position); a padding row, a row past the slab
  // or past the batch reads the first element of the batch and is not used
  int st_smp[NR], st_l[NR], st_sm[NR];
  bool st_row[NR], st_ok[NR];
  auto set_rows = [&](int s0) {
#pragma unroll
    for (int i = 0; i < NR; ++i) {
      const int row = (tid & 31) + 32 * i, sm = row / RS, l = row - sm * RS - 2, smp = s0 + sm;
      st_row[i] = row < SROWS;
      st_ok[i] = st_row[i] && smp < m.n && l >= 0 && l < L;
      st_sm[i] = st_row[i] ? sm : 0;
      st_smp[i] = st_ok[i] ? smp : 0;
      st_l[i] = st_ok[i] ? l : 0;
    }
  };
  // the raw rows of (item, chunk): item = (channel block, slab row): the 8 channels of one position (32 contiguous bytes of a blocked tensor);
  // a thread has <= 2 blocks x NR rows.  They are REQUESTED one stage ahead -- behind the previous stage's conversion, so that their
  // latency passes under its GEMM and tail (the weight ring's loads of a stage are issued before, and loads return in order)
  float4 v[NBH][NR][2];
  auto chunk_blocks = [&](int ch) {                       // channel blocks of chunk ch (the k1 conv's chunk is always four K chunks wide)
    const int cc = K == 1 ? m.kch : min(m.kch, cin - ch * m.kch);
    return 4 * ((cc + 31) / 32);
  };
  auto request_rows = [&](int ch) {
    const int c_lo = ch * m.kch, NB = chunk_blocks(ch);
#pragma unroll
    for (int h = 0; h < NBH; ++h) {
      const int blk = (tid >> 5) + 8 * h, c = c_lo + 8 * blk;   // (c1 is a multiple of 8: the block lies in one source)
      if (blk >= NB) continue;
      const bool live = a.in_cl ? c == 0 : c < cin, first = c < a.c1;
      const float* const src = a.in_cl ? a.x1 : first ? a.x1 + (size_t)c * L : a.x2 + (size_t)(c - a.c1) * L;
      const int cw = first ? a.c1 : a.c2;                  // channels of the source: a sample is cw x L elements
#pragma unroll
      for (int i = 0; i < NR; ++i) {
        // blocked: ((smp cw / 8 + c / 8) L + l) 8; the trajectory [n][L][4]: channels 0 .. 3 are one 16-byte load
        const float* const q = !live ? a.x1 : a.in_cl ? src + ((size_t)st_smp[i] * L + st_l[i]) * 4 : src + (size_t)st_smp[i] * cw * L + st_l[i] * 8;
        v[h][i][0] = live ? *reinterpret_cast<const float4*>(q) : make_float4(0.f, 0.f, 0.f, 0.f);
        v[h][i][1] = live && !a.in_cl ? *reinterpret_cast<const float4*>(q + 4) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
  };
  // ---- GEMM over the channel chunks
  constexpr int WPT = 4 / MTW;                             // waves that share an n-tile (MTW < 4: they split its M tiles)
  const int nt0 = (wave / WPT) * NTW;                      // first n-tile of the wave
  const int mt0 = wave % WPT;                              // its M tiles: mt0, mt0 + WPT, ...
  const int row = lane & 15, g = lane >> 4;
  int arow[MTW];                                           // slab row of the lane's A row in its M tile i at tap 0: position S lo - K / 2
  int csm[MTW];                                            // sample (of the workgroup) of the lane's four C/D rows 4 g .. 4 g + 3 of M tile i
  float inv_prev[MTW];                                     // 1 / (the current chunk's scale) of that sample
#pragma unroll
  for (int i = 0; i < MTW; ++i) {
    const int r64 = 16 * (mt0 + i * WPT) + row;            // (sample, output row) of the 64
    arow[i] = (r64 >> lsh) * RS + S * (r64 & (LR - 1)) + 2 - K / 2;
    csm[i] = (16 * (mt0 + i * WPT) + 4 * g) >> lsh;
    inv_prev[i] = 1.f;
  }
  f32x4 acc[NTW][MTW];
  // the weight ring: B fragments of step st of the wave's n-tiles nt0 + t (wp: the wave's first fragment, tstride: one n-tile further)
  u32x4 b[RD][NTW][2];
  auto load_b = [&](const u32x4* wp, size_t tstride, int slot, int st) {
#pragma unroll
    for (int t = 0; t < NTW; ++t) {
      b[slot][t][0] = wp[t * tstride + (size_t)st * 128];
      b[slot][t][1] = wp[t * tstride + (size_t)st * 128 + 64];
    }
  };
  auto ring_start = [&](const u32x4* wp, size_t tstride) {
#pragma unroll
    for (int j = 0; j < RD; ++j) load_b(wp, tstride, j, j);
  };
  // the GEMM of one chunk: `steps` = K x KCj steps (tap, kc), tap-major, over the slab's KCj x 4 channel blocks (PS: bytes of a piece)
  auto gemm = [&](const u32x4* wp, size_t tstride, int steps, int KCj, int PS) {
    auto group = [&](int base, auto refill) {              // RD steps: slot j holds step base + j and is refilled with step base + j + RD
#pragma unroll
      for (int j = 0; j < RD; ++j) {
        const int st = base + j, tap = st / KCj, kc = st - tap * KCj;
        const char* const ablk = slab + ((size_t)(KCj * g + kc) * SROWS + tap) * 16;
        u32x4 af[MTW][2];
#pragma unroll
        for (int i = 0; i < MTW; ++i) {
          af[i][0] = *reinterpret_cast<const u32x4*>(ablk + arow[i] * 16);
          af[i][1] = *reinterpret_cast<const u32x4*>(ablk + PS + arow[i] * 16);
        }
#pragma unroll
        for (int i = 0; i < MTW; ++i)
#pragma unroll
          for (int t = 0; t < NTW; ++t) vb_three<false>(acc[t][i], af[i], b[j][t]);
        if (decltype(refill)::value) load_b(wp, tstride, j, st + RD);
      }
    };
    // (the last group peeled: every load of the loop is unconditional, so the waits count loads instead of draining them)
    for (int base = 0; base < steps - RD; base += RD) group(base, std::true_type{});
    group(steps - RD, std::false_type{});
  };
  // (the widest slice keeps no rows in flight across its GEMM: the registers are the weight ring's -- its stages are GEMM-bound)
  constexpr bool AHEAD = NTW == 1 && KIND != 4;          // (nor does the two-conv block: its rows would be held through both tails)
  int item = blockIdx.x, ch = 0, s0 = item * SPW;
  set_rows(s0);
  if (AHEAD) request_rows(0);
  __syncthreads();                                         // smax is zero
  for (unsigned seq = 0;; ++seq) {                         // the stages (item, chunk) of this workgroup
    const int NB = chunk_blocks(ch), KCj = NB / 4;
    const int PS = NB * SROWS * 16;
    unsigned* const mxs = smax + 8 * (seq & 1);
    if (seq) __syncthreads();                              // every wave is done reading the previous stage's slab / output tile
    if (ch == 0) {
      if (KIND == 4 && tid < 8) smax[16 + tid] = 0u;       // (the maxima of the block's hidden tensor: the previous item is done with them)
#pragma unroll
      for (int i = 0; i < MTW; ++i) {
        inv_prev[i] = 1.f;
#pragma unroll
        for (int t = 0; t < NTW; ++t) acc[t][i] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
    // the weight ring's first steps are requested before the staging: their latency passes under it
    const int steps = K * KCj;                             // (tap, kc), tap-major: a multiple of the ring's RD slots
    // the wave's B fragments of step st: n-tile nt0 + t, pieces q
    const u32x4* const wp = reinterpret_cast<const u32x4*>(m.wpk) + (size_t)ch * m.stride + (size_t)(c0 / 16 + nt0) * steps * 128 + lane;
    const size_t tstride = (size_t)steps * 128;            // one n-tile further
    ring_start(wp, tstride);
    if (!AHEAD) request_rows(ch);
    {
      // the samples' maxima over the chunk
#pragma unroll
      for (int i = 0; i < NR; ++i) {
        float mx = 0.f;
#pragma unroll
        for (int h = 0; h < NBH; ++h) {
          if ((tid >> 5) + 8 * h >= NB) continue;
          const float4 p = v[h][i][0], q = v[h][i][1];
          mx = fmaxf(mx, fmaxf(fmaxf(fmaxf(fabsf(p.x), fabsf(p.y)), fmaxf(fabsf(p.z), fabsf(p.w))),
                               fmaxf(fmaxf(fabsf(q.x), fabsf(q.y)), fmaxf(fabsf(q.z), fabsf(q.w)))));
        }
        if (st_ok[i] && mx > 0.f) atomicMax(mxs + st_sm[i], __float_as_uint(mx));
      }
      __syncthreads();
      MCONV_T(0)
      if (tid < 8) smax[8 * ((seq + 1) & 1) + tid] = 0u;   // (the other stage's maxima: every thread has used them by now)
#pragma unroll
      for (int h = 0; h < NBH; ++h) {
        const int blk = (tid >> 5) + 8 * h;
        if (blk >= NB) continue;
#pragma unroll
        for (int i = 0; i < NR; ++i) {
          if (!st_row[i]) continue;
          const float sc = st_ok[i] ? dyn_scale(__uint_as_float(mxs[st_sm[i]])).s : 0.f;
          const float4 p = st_ok[i] ? v[h][i][0] : make_float4(0.f, 0.f, 0.f, 0.f), q = st_ok[i] ? v[h][i][1] : make_float4(0.f, 0.f, 0.f, 0.f);
          const F16Pair p0 = f16_split2(p.x * sc, p.y * sc), p1 = f16_split2(p.z * sc, p.w * sc), p2 = f16_split2(q.x * sc, q.y * sc),
                        p3 = f16_split2(q.z * sc, q.w * sc);
          const size_t o = ((size_t)blk * SROWS + (tid & 31) + 32 * i) * 16;
          *reinterpret_cast<uint4*>(slab + o) = make_uint4(p0.hi, p1.hi, p2.hi, p3.hi);
          *reinterpret_cast<uint4*>(slab + PS + o) = make_uint4(p0.lo, p1.lo, p2.lo, p3.lo);
        }
      }
    }
    // the accumulators pass into the new chunk's units
#pragma unroll
    for (int i = 0; i < MTW; ++i) {
      const DynScale ds = dyn_scale(__uint_as_float(mxs[csm[i]]));
      if (ch) {
        const float r = ds.s * inv_prev[i];
#pragma unroll
        for (int t = 0; t < NTW; ++t) acc[t][i] *= r;
      }
      inv_prev[i] = ds.inv;
    }
    // the next stage's rows are requested now (v is free), to land under this stage's GEMM and tail
    const bool last_chunk = ch + 1 == m.n_chunks;
    const int n_item = last_chunk ? item + (int)gridDim.x : item, n_ch = last_chunk ? 0 : ch + 1;
    const bool more = n_item < n_items;
    if (more) {
      if (last_chunk) set_rows(n_item * SPW);
      if (AHEAD) request_rows(n_ch);
    }
    __syncthreads();
    MCONV_T(1)
    gemm(wp, tstride, steps, KCj, PS);
    MCONV_T(2)
    if (last_chunk) {
      if (KIND != 0 && KIND != 4) {
        // ---- plain convs: column scale x sample scale, + bias, stored from the accumulators (C/D layout: lane = column lane & 15, rows 4 g ..
        // 4 g + 3 of the M tile = four consecutive output rows of one sample) into the blocked output: the 16 lanes of a row write 64
        // contiguous bytes (two channel blocks; the transposed conv: one block at the positions 2 m and 2 m + 1)
#pragma unroll
        for (int t = 0; t < NTW; ++t) {
          const int col = c0 + 16 * (nt0 + t) + row, co = KIND == 3 ? col >> 1 : col;
          const float kc_ = m.isc[col], bs = a.bias[co];
#pragma unroll
          for (int i = 0; i < MTW; ++i) {
            const int r64 = 16 * (mt0 + i * WPT) + 4 * g, lo = r64 & (LR - 1), smp = s0 + csm[i];
            const float k = kc_ * inv_prev[i];
            if (smp >= m.n) continue;
            float* const dst = a.y + bl_off(smp, a.c_out, a.l_out, co, KIND == 3 ? 2 * lo + (col & 1) : lo);
#pragma unroll
            for (int e = 0; e < 4; ++e) dst[(KIND == 3 ? 16 : 8) * e] = fmaf(acc[t][i][e], k, bs);
          }
        }
        MCONV_T(5)
      } else {
        // ---- Conv1dBlock tail.  A thread owns rows 4 rq .. 4 rq + 3 (one sample: rq = tid % 16) x the NIT adjacent channels cl NIT .. of the
        // slice (cl = tid / 16)
        float* const outs = reinterpret_cast<float*>(smem);      // [cs][OST] conv output (64 rows + 4 of padding: conflict-free column writes)
        constexpr int NIT = NTW * MTW;                           // = cs / 16
        const int rq = tid & 15, cl = tid >> 4, r0 = 4 * rq, tsm = r0 >> lsh, tl = r0 & (L - 1), tsmp = s0 + tsm, tc = c0 + cl * NIT;
        const int cpg = a.c_out / N_GROUPS, clu = cpg / NIT;     // channel lanes (16 apart) per group: 2, 4, 8 or 16
        // the sum of a (sample, group) -- cpg channels x L positions -- is DEFINED as: per channel the four rows of a quad ((x0 + x1) + (x2 +
        // x3)); a balanced tree over the channel index (within the thread, then lanes 16 and 32 apart, then waves); then a balanced tree
        // over the sample's row quads (lanes 1, 2, 4, 8 apart) -- whatever the slice width
        auto group_sum = [&](float (&s)[NIT]) -> float {
#pragma unroll
          for (int w = 1; w < NIT; w *= 2)
#pragma unroll
            for (int k = 0; k < NIT; k += 2 * w) s[k] += s[k + w];
          float v = s[0];
          v += __shfl_xor(v, 16);
          if (clu >= 4) v += __shfl_xor(v, 32);
          if (clu >= 8) {                                        // the group spans 2 or 4 waves
            if (lane < 16) red[16 * wave + lane] = v;
            __syncthreads();
            const int w0 = clu >= 16 ? 0 : wave & 2;
            v = red[16 * w0 + rq] + red[16 * (w0 + 1) + rq];
            if (clu >= 16) v = v + (red[32 + rq] + red[48 + rq]);
            __syncthreads();
          }
          v += __shfl_xor(v, 1);
          if (L >= 16) v += __shfl_xor(v, 2);
          if (L >= 32) v += __shfl_xor(v, 4);
          if (L >= 64) v += __shfl_xor(v, 8);
          return v;
        };
        // accumulators (in units of 1 / inv[i]) -> conv output + bias -> GroupNorm -> Mish -> + addend (per channel, or per element from a
        // blocked tensor) -> o[row][channel] of the thread's 4 x NIT patch.  The global operands are requested first, so that their latency
        // passes under the exchange
        auto block_tail = [&](const float* bias, const float* gamma, const float* beta, const float* isc, const float* add_c,
                              const float* add_t, const float (&inv)[MTW], float (&o)[4][NIT]) {
          float gm[NIT], bt[NIT], ad[4][NIT];                    // gamma, beta; the addend per (row, channel)
#pragma unroll
          for (int k = 0; k < NIT; ++k) {
            gm[k] = gamma[tc + k];
            bt[k] = beta[tc + k];
          }
          if (add_c) {
#pragma unroll
            for (int k = 0; k < NIT; ++k) ad[0][k] = ad[1][k] = ad[2][k] = ad[3][k] = add_c[tc + k];
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              if (add_t && tsmp < m.n) {
                ld_run<NIT>(ad[e], add_t + bl_off(tsmp, a.c_out, L, tc, tl + e));
              } else {
#pragma unroll
                for (int k = 0; k < NIT; ++k) ad[e][k] = 0.f;
              }
            }
          }
          float kc_[NTW], bs_[NTW];
#pragma unroll
          for (int t = 0; t < NTW; ++t) {
            kc_[t] = isc[c0 + 16 * (nt0 + t) + row];
            bs_[t] = bias[c0 + 16 * (nt0 + t) + row];
          }
          __syncthreads();                                       // the slab is dead: its memory becomes the output tile
          // accumulators -> outs[c][r64] (C/D layout: lane = column lane & 15, rows 4 g .. 4 g + 3 of the M tile), scaled back, + bias
#pragma unroll
          for (int t = 0; t < NTW; ++t) {
            const int ocl = 16 * (nt0 + t) + row;
#pragma unroll
            for (int i = 0; i < MTW; ++i) {
              const int r64 = 16 * (mt0 + i * WPT) + 4 * g;
              const float k = kc_[t] * inv[i], bs = bs_[t];
              *reinterpret_cast<float4*>(outs + ocl * OST + r64) =
                  make_float4(fmaf(acc[t][i][0], k, bs), fmaf(acc[t][i][1], k, bs), fmaf(acc[t][i][2], k, bs), fmaf(acc[t][i][3], k, bs));
            }
          }
          __syncthreads();
          MCONV_T(3)
          float4 x[NIT];
#pragma unroll
          for (int k = 0; k < NIT; ++k) x[k] = *reinterpret_cast<const float4*>(outs + (cl * NIT + k) * OST + r0);
          const float per = (float)(cpg << lsh);
          float s[NIT];
#pragma unroll
          for (int k = 0; k < NIT; ++k) s[k] = (x[k].x + x[k].y) + (x[k].z + x[k].w);
          const float mean = group_sum(s) / per;                 // two passes, as the reference: the mean, then the squared deviations
#pragma unroll
          for (int k = 0; k < NIT; ++k) {
            const float d0 = x[k].x - mean, d1 = x[k].y - mean, d2 = x[k].z - mean, d3 = x[k].w - mean;
            s[k] = (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
          }
          const float rstd = 1.f / sqrtf(group_sum(s) / per + 1e-5f);
          MCONV_T(4)
          // normalise + Mish + addend (the fused kernel's arithmetic, gn_mish.h)
#pragma unroll
          for (int k = 0; k < NIT; ++k) {
            const GnCoef cf = gn_coef(mean, rstd, gm[k], bt[k]);
            const f32x2_t lo = gn_mish2(f32x2_t{x[k].x, x[k].y}, cf, f32x2_t{ad[0][k], ad[1][k]});
            const f32x2_t hi = gn_mish2(f32x2_t{x[k].z, x[k].w}, cf, f32x2_t{ad[2][k], ad[3][k]});
            o[0][k] = lo.x; o[1][k] = lo.y; o[2][k] = hi.x; o[3][k] = hi.y;
          }
        };
        float o[4][NIT];
        if (KIND == 0) {
          block_tail(a.bias, a.gamma, a.beta, m.isc, a.add_c, a.add_t, inv_prev, o);
        } else {
          // ---- KIND 4, a whole ResidualTemporalBlock (cs = c_out: one slice).  The first Conv1dBlock's output + time bias stays in the
          // workgroup: it becomes the second conv's A slab (fp16 pieces under its own per-sample scale: the maximum over the thread patches,
          // LDS atomics as in the staging) -- the arithmetic of the two-launch form, without the tensor's trip through memory
          block_tail(a.bias, a.gamma, a.beta, m.isc, a.add_c, nullptr, inv_prev, o);
          const int KC2 = a.c_out / 32, NB2 = 4 * KC2, PS2 = NB2 * SROWS * 16, steps2 = K * KC2;
          const u32x4* const wp2 = reinterpret_cast<const u32x4*>(m.wpk2) + (size_t)nt0 * steps2 * 128 + lane;
          if (NTW == 1) ring_start(wp2, (size_t)steps2 * 128);   // (the widest slice: behind the conversion, its patch is 32 registers)
          unsigned* const mx2 = smax + 16;
          float mx = 0.f;
#pragma unroll
          for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int k = 0; k < NIT; ++k) {
              if (tsmp >= m.n) o[e][k] = 0.f;                    // (a sample past the batch: zeros, as the staging gives)
              mx = fmaxf(mx, fabsf(o[e][k]));
            }
          if (mx > 0.f) atomicMax(mx2 + tsm, __float_as_uint(mx));
          __syncthreads();                                       // the maxima are complete, and every thread has read its patch of the tile
          {
            const float sc = dyn_scale(__uint_as_float(mx2[tsm])).s;
            // the thread's NIT channels of row e: 2 NIT bytes at channel offset tc % 8 of block tc / 8 (tc = cl NIT: c0 = 0)
            char* const dst = slab + ((size_t)(tc >> 3) * SROWS + tsm * RS + 2 + tl) * 16 + (tc & 7) * 2;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              unsigned hi[NIT / 2 > 0 ? NIT / 2 : 1], lo[NIT / 2 > 0 ? NIT / 2 : 1];
#pragma unroll
              for (int k = 0; k + 1 < NIT; k += 2) {
                const F16Pair pr = f16_split2(o[e][k] * sc, o[e][k + 1] * sc);
                hi[k / 2] = pr.hi;
                lo[k / 2] = pr.lo;
              }
              if constexpr (NIT == 8) {
                *reinterpret_cast<uint4*>(dst + e * 16) = make_uint4(hi[0], hi[1], hi[2], hi[3]);
                *reinterpret_cast<uint4*>(dst + PS2 + e * 16) = make_uint4(lo[0], lo[1], lo[2], lo[3]);
              } else if constexpr (NIT == 4) {
                *reinterpret_cast<uint2*>(dst + e * 16) = make_uint2(hi[0], hi[1]);
                *reinterpret_cast<uint2*>(dst + PS2 + e * 16) = make_uint2(lo[0], lo[1]);
              } else {
                *reinterpret_cast<unsigned*>(dst + e * 16) = hi[0];
                *reinterpret_cast<unsigned*>(dst + PS2 + e * 16) = lo[0];
              }
            }
            // the padding rows (two either side of a sample) of every block, both pieces
            for (int i = tid; i < SPW * 4 * NB2 * 2; i += 256) {
              const int h = i & 3, sm = (i >> 2) % SPW, bq = (i >> 2) / SPW;        // bq = piece * NB2 + block
              *reinterpret_cast<uint4*>(slab + ((size_t)bq * SROWS + sm * RS + (h < 2 ? h : L + h)) * 16) = make_uint4(0u, 0u, 0u, 0u);
            }
          }
          if (NTW != 1) ring_start(wp2, (size_t)steps2 * 128);
          float inv2[MTW];
#pragma unroll
          for (int i = 0; i < MTW; ++i) {
            inv2[i] = dyn_scale(__uint_as_float(mx2[csm[i]])).inv;
#pragma unroll
            for (int t = 0; t < NTW; ++t) acc[t][i] = f32x4{0.f, 0.f, 0.f, 0.f};
          }
          __syncthreads();                                       // the second conv's slab is complete
          gemm(wp2, (size_t)steps2 * 128, steps2, KC2, PS2);
          block_tail(m.bias2, m.gamma2, m.beta2, m.isc2, nullptr, a.add_t, inv2, o);
        }
        // -> y, blocked: a row's NIT channels are one run
        if (tsmp < m.n) {
#pragma unroll
          for (int e = 0; e < 4; ++e) st_run<NIT>(a.y + bl_off(tsmp, a.c_out, L, tc, tl + e), o[e]);
        }
        MCONV_T(5)
      }
    }
    if (!more) break;
    item = n_item;
    ch = n_ch;
    s0 = item * SPW;
  }
#ifdef MCONV_TIMING
  if (tid == 0) {
    unsigned long long* t = g_mconv_clk[KIND][lsh_in - 3][NTW * MTW];
    for (int i = 0; i < 6; ++i) atomicAdd(t + i, (unsigned long long)clk_[i]);
    atomicAdd(t + 6, (unsigned long long)(clock64() - first_));
    atomicAdd(t + 7, (unsigned long long)((n_items - 1 - (int)blockIdx.x) / (int)gridDim.x + 1));
  }
#endif
}

}  // namespace

}  // namespace mmd
