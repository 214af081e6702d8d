// TemporalUnet forward for gfx950 (MI355X), the whole network in ONE launch (unet_kernel).  Every Conv1d /
// ConvTranspose1d of the reference network (mmd/models/diffusion_models/temporal_unet.py:121-174,
// mmd/models/layers/layers.py:261-358) is an fp32-accurate GEMM on the matrix pipe, with GroupNorm + Mish + time-bias /
// residual fused into the epilogue:
//   * f16x2: an fp32 operand is split into two fp16 pieces (round to nearest, twice) and a product is three
//     v_mfma_f32_16x16x32_f16 (a1*w0 + a0*w1 + a0*w0) with fp32 accumulation -- 1/5 of the fp32 MFMA's pipe time, at
//     least its accuracy.  Power-of-two scales keep the pieces inside fp16's range: per output channel for weights
//     (host), static for the inputs of an RTB's second conv (bounded by GroupNorm), dynamic per sample for the
//     residual stream (dyn_scale); all of them leave through the GroupNorm epilogue's coefficients.
//   * every conv is a DIRECT convolution (taps = row-shifted views of an fp16 slab): downs.0 and ups.1 + final block
//     wave-private (wave = sample, no workgroup barriers inside the stage), downs.1 / downs.2 + mid / ups.0 on workgroup slabs
//     (a wave owns 1-2 n-tiles x 2-4 samples); strided tails read their slab at stride 2, transposed tails = two parity passes.
//   * no register spills (a reload waits for every weight load in flight): downs.2's residual tile is parked
//     lane-privately in LDS; epilogue parameters and the residual conv's weights are requested ahead of their use.
//
// Layout.  The trajectory tensor is channels-last [n_traj, 64, 4] fp32 in HBM on both sides (no transposes).  A
// workgroup (4 waves) owns 4 whole samples for the entire forward: activations live in LDS slabs (fp32 row form
// [sample][L+4][C+2] for downs.2's input; fp16 row form [piece][lane group][K chunk][row][8 ch], RdGeo / RlGeo / RwGeo) and
// in register tiles; the two skip connections wait in registers for the up path; nothing but the input, the output
// and the weights touches HBM/L2.  In the 16x16 C/D layout a lane holds 4 consecutive positions of one channel per tile, so a GroupNorm group is a few lanes of one DPP row (x row blocks): the statistics are
// in-register + cross-lane reductions.  Weights are pre-packed on the host in MFMA B-fragment order (fp16 pairs) and fetched straight from L2 through a register ring (no LDS
// staging: a B element is used once per workgroup).  HISTORY.md section 3.1 has the measurements behind each choice.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>

#include "../../include/mmd_amd.h"
#include "../../include/mmd_amd_debug.h"
#include "common.h"
#include "f16x2.h"
#include "gn_mish.h"
#include "guide_dev.h"
#include "unet_spec.h"

// Two precisions from this one source.  As included by unet.hip everything below is the f16x2 arithmetic described above (namespace mmd,
// N_PIECES = 2).  unet_f16.hip includes it under MMD_UNET_F16 (mmd_unet_options.precision = MMD_UNET_PRECISION_F16): the same stages,
// slabs, weight packs, scales and epilogues in namespace mmd::f16 -- kernels with symbols of their own -- with ONE fp16 piece per
// operand: f16_split2 / vb_three are shadowed by one-piece forms, the low pieces are neither stored (MMD_LO) nor zeroed nor staged, and
// what still reads them (rd_load_a / rd_load_b, piece q = 1) is dead code to the compiler.
#ifdef MMD_UNET_F16
#define MMD_LO(...)
namespace mmd {
namespace f16 {
constexpr int N_PIECES = 1;
struct F16Pair { unsigned hi; };
__device__ __forceinline__ F16Pair f16_split2(float v0, float v1) {
  return F16Pair{__builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{v0, v1}, f16x2))};   // v_cvt_pk_f16_f32 (round to nearest even)
}
// one K = 32 chunk of one accumulator stream: a0 b0 (program order kept, as the triple's is)
template <bool ZERO>
__device__ __forceinline__ void vb_three(f32x4& x, const u32x4 (&a)[2], const u32x4 (&b)[2]) {
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  x = mfma_h(a[0], b[0], ZERO ? z : x);
  __builtin_amdgcn_sched_barrier(0);
}
#else
#define MMD_LO(...) __VA_ARGS__
namespace mmd {
constexpr int N_PIECES = 2;
#endif

// final Conv1dBlock(32->32, k5) + Conv1d(32->4, k1) of the network
struct FinalArgs {
  float* out;             // eps [n, 64, 4]
  const uint4* w5;        // f16x2 pack of the k5 conv (interleaved column pairs)
  const float* rec5;      // [16] epilogue records of the k5 conv (channel pairs: bias, GroupNorm weight / bias, inverse scales of w5)
  float act;              // static power-of-two scale of the block's output activations = the 1x1 conv's f16x2 input
  const uint4* w1_bf;     // f16x2 pack of the 1x1 conv (one n-tile, columns >= 4 zero)
  const float* rec1;      // [4] records of the 1x1 conv's output channels: {bias, inverse channel scale of w1_bf / act, 0, 0}
};

// GroupNorm-epilogue parameters of a conv for the lane's NT adjacent channels.  They are REQUESTED BEFORE the conv's taps (the
// stage bodies call epi_load ahead of the weight ring): read inside the epilogue they cost every conv an exposed L2 round trip
// (~0.5 us, 25 times per forward) -- nothing else is in flight at that point and the statistics need the bias at once.
template <int NT> struct Epi { float b[NT], g[NT], be[NT], is[NT], tb[NT]; };
template <int NT>
__device__ __forceinline__ Epi<NT> epi_load(const float* b, const float* g, const float* be, const float* tb, const float* isc, int c0) {
  Epi<NT> e;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    e.b[t] = b[c0 + t];
    e.g[t] = g[c0 + t];
    e.be[t] = be[c0 + t];
    e.is[t] = isc ? isc[c0 + t] : 1.f;
    e.tb[t] = tb ? tb[c0 + t] : 0.f;
  }
  return e;
}
// The kernels below read these parameters from RECORD TABLES the packer writes (unet.hip, push_records): one record per channel unit of
// NT adjacent channels (the lane's c0 .. c0 + NT - 1: unit c0 / NT), its fields in order, each field's NT channels side by side, zero
// padded to whole float4 -- {b0, b1, g0, g1, be0, be1, is0, is1} for NT = 2 -- so a lane fetches a conv's constants with one
// global_load_dwordx4 per 16 bytes where the separate arrays took one narrow load per field and channel (a whole vector-memory
// instruction each, counted by the same in-order vmcnt as the weight ring).  The values are the floats the arrays held.
constexpr int rec_floats(int fields, int nt) { return (fields * nt + 3) / 4 * 4; }
template <int FIELDS, int NT> struct Rec {
  float v[FIELDS * NT];
  __device__ __forceinline__ float at(int field, int t) const { return v[field * NT + t]; }
};
// (whole float4 first; the record's last 1 - 3 floats in front of its padding as one narrower load, so no register waits for a zero)
template <int FIELDS, int NT>
__device__ __forceinline__ Rec<FIELDS, NT> rec_load(const float* table, unsigned unit) {
  typedef float f32x3 __attribute__((ext_vector_type(3)));
  constexpr int F = FIELDS * NT, Q = F / 4, REM = F % 4;
  const float* p = table + unit * (unsigned)rec_floats(FIELDS, NT);
  Rec<FIELDS, NT> r;
#pragma unroll
  for (int i = 0; i < Q; ++i) {
    const f32x4 q = *reinterpret_cast<const f32x4*>(p + 4 * i);
#pragma unroll
    for (int j = 0; j < 4; ++j) r.v[4 * i + j] = q[j];
  }
  if constexpr (REM == 3) {
    const f32x3 q = *reinterpret_cast<const f32x3*>(p + 4 * Q);
    r.v[4 * Q] = q[0]; r.v[4 * Q + 1] = q[1]; r.v[4 * Q + 2] = q[2];
  } else if constexpr (REM == 2) {
    const float2 q = *reinterpret_cast<const float2*>(p + 4 * Q);
    r.v[4 * Q] = q.x; r.v[4 * Q + 1] = q.y;
  } else if constexpr (REM == 1) {
    r.v[4 * Q] = p[4 * Q];
  }
  return r;
}
// the time bias of channels c0 .. c0 + NT - 1 (row t of the time table: the one epilogue parameter that is not a constant of the model),
// one load per lane
template <int NT>
__device__ __forceinline__ void tb_load(float (&d)[NT], const float* tb, unsigned c0) {
  static_assert(NT == 1 || NT == 2, "a lane owns one channel or an adjacent (even, odd) pair");
  if constexpr (NT == 2) {
    const float2 v = *reinterpret_cast<const float2*>(tb + c0);   // (c0 even, rows and blocks of the table start at even columns)
    d[0] = v.x; d[1] = v.y;
  } else {
    d[0] = tb[c0];
  }
}
// fields 0 .. 3 of a record = a GroupNorm epilogue's constants; tb: the conv's time-bias row or null
template <int NT, int FIELDS>
__device__ __forceinline__ Epi<NT> epi_of(const Rec<FIELDS, NT>& r, const float* tb, unsigned c0) {
  Epi<NT> e;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    e.b[t] = r.at(0, t);
    e.g[t] = r.at(1, t);
    e.be[t] = r.at(2, t);
    e.is[t] = r.at(3, t);
    e.tb[t] = 0.f;
  }
  if (tb) tb_load<NT>(e.tb, tb, c0);
  return e;
}
template <int NT>
__device__ __forceinline__ Epi<NT> epi_rec(const float* table, const float* tb, unsigned c0) {
  return epi_of<NT>(rec_load<4, NT>(table, c0 / NT), tb, c0);
}
// ... of a stage's first conv A, whose record carries the 1x1 residual conv's bias and inverse weight scales behind them (fields 4, 5)
template <int NT>
__device__ __forceinline__ Epi<NT> epi_rec_res(const float* table, const float* tb, unsigned c0, float (&br)[NT], float (&isr)[NT]) {
  const Rec<6, NT> r = rec_load<6, NT>(table, c0 / NT);
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    br[t] = r.at(4, t);
    isr[t] = r.at(5, t);
  }
  return epi_of<NT>(r, tb, c0);
}
// A tail conv's record: its bias and the inverse channel scales of its NP packs (Downsample1d: one; ConvTranspose1d: the two parity passes)
template <int NT, int NP> struct TailRec { float bt[NT], is[NP][NT]; };
template <int NT, int NP>
__device__ __forceinline__ TailRec<NT, NP> tail_rec(const float* table, unsigned c0) {
  const Rec<1 + NP, NT> r = rec_load<1 + NP, NT>(table, c0 / NT);
  TailRec<NT, NP> e;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    e.bt[t] = r.at(0, t);
#pragma unroll
    for (int p = 0; p < NP; ++p) e.is[p][t] = r.at(1 + p, t);
  }
  return e;
}

// The lane's value combined with the same lane of the neighbouring 16-lane row (xor 16) / of the other wave half (xor 32):
// v_permlane16_swap / v_permlane32_swap (gfx950) exchange the odd rows of one operand with the even rows of the other, so with
// both operands = v the two results are (row 0, row 0, row 2, row 2) and (row 1, row 1, row 3, row 3) -- one VALU
// instruction instead of a ds_bpermute round trip through the LDS in the dependent chain of every GroupNorm reduction.
struct RowPair { float a, b; };
__device__ __forceinline__ RowPair rows_xor16(float v) {
  const unsigned u = __builtin_bit_cast(unsigned, v);
  const auto r = __builtin_amdgcn_permlane16_swap(u, u, false, false);
  return RowPair{__builtin_bit_cast(float, (unsigned)r[0]), __builtin_bit_cast(float, (unsigned)r[1])};
}
__device__ __forceinline__ RowPair rows_xor32(float v) {
  const unsigned u = __builtin_bit_cast(unsigned, v);
  const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  return RowPair{__builtin_bit_cast(float, (unsigned)r[0]), __builtin_bit_cast(float, (unsigned)r[1])};
}
__device__ __forceinline__ float add_xor16(float v) { const RowPair r = rows_xor16(v); return r.a + r.b; }
__device__ __forceinline__ float add_xor32(float v) { const RowPair r = rows_xor32(v); return r.a + r.b; }
// The maximum of two floats whose SIGN BIT IS CLEAR (+0, positive denormal / normal, +inf, a NaN behind fabsf) as the unsigned maximum of
// their bit patterns: on such floats the integer order is the float order, and +inf / NaN (biased exponent 255) stay on top, which is all
// dyn_scale reads.  fmaxf on operands that arrive through a bit cast (DPP, permlane, LDS) costs a NaN-quieting v_max_f32 x, x, x per operand
// and keeps a DPP step from folding into the max; this is one v_max_u32 (v_max_u32_dpp, v_max3_u32).  NOT for an operand that may carry a sign
// bit, -0.0 included: 0x80000000 is the largest unsigned value but the smallest float magnitude.
__device__ __forceinline__ float max_nn(float a, float b) {
  const unsigned ua = __builtin_bit_cast(unsigned, a), ub = __builtin_bit_cast(unsigned, b);
  return __builtin_bit_cast(float, __builtin_elementwise_max(ua, ub));   // (the intrinsic: a compare + select written out stays one)
}
// (v >= 0 in all of the reductions below: they only ever see maxima of absolute values)
__device__ __forceinline__ float max_xor16(float v) { const RowPair r = rows_xor16(v); return max_nn(r.a, r.b); }   // (both rows' v >= 0)
__device__ __forceinline__ float max_xor32(float v) { const RowPair r = rows_xor32(v); return max_nn(r.a, r.b); }   // (both halves' v >= 0)

template <int CTRL>
__device__ __forceinline__ float dpp_max(float v) {   // max(v, v[DPP-permuted lane]) in one VALU op (v >= 0 in every lane)
  return max_nn(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true)));
}
__device__ __forceinline__ float row_max16(float v) {      // max over the 16 lanes of a DPP row, in all of them (v >= 0)
  v = dpp_max<0xB1>(v);
  v = dpp_max<0x4E>(v);
  v = dpp_max<0x141>(v);
  v = dpp_max<0x140>(v);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {       // max over the wave's 64 lanes, in all of them (v >= 0)
  v = row_max16(v);
  v = max_xor16(v);
  return max_xor32(v);
}
constexpr int MX_SLOTS = 8;                                  // partial maxima per sample (waves x lane groups sharing a sample)
constexpr int MX_REGION = 4 * MX_SLOTS;                      // region 0: the conv being prepared; 1 / 2: downs.2's skip2 / the
constexpr int MX_FLOATS = 3 * MX_REGION;                     // mid blocks' output, kept for ups.0's conv A

// acc[mt] += A(slab rows, taps x CP channels) * B(packed).  abase[mt] is the lane's slab offset of (row, k=lane>>5)
// for tap 0; tap t reads STR floats further.  wp points at this lane's float4 of the first k-group.
// B fragments are prefetched FOUR k-groups (32 MFMAs = 2048 cycles) ahead through a 4-register ring so the L2
// latency of a weight fetch never sits in front of the MFMA that consumes it; pack_b pads every packed tensor with 4
// zero groups so the ring may over-read unconditionally.
// A compiler-level memory barrier right after a ring refill: the weight loads are read-only, so LLVM is otherwise free to
// sink them down to their first use (one k-group later: the L2 latency then sits in front of the MFMA again).
// The machine scheduler gets a full barrier at the same point, or it hoists the VALU consumers of an LDS read up to the
// read (and with them the s_waitcnt), which exposes the LDS latency once per k-step.
#ifdef MMD_NO_PIN                        // (tools/ubench/fatwave_conv.hip: the scheduler is steered by sched_group_barrier there)
#define MMD_PIN_LOADS() do { } while (0)
#else
#define MMD_PIN_LOADS()                 \
  do {                                  \
    asm volatile("" ::: "memory");      \
    __builtin_amdgcn_sched_barrier(0);  \
  } while (0)
#endif

// Phase tracing (side builds with -DMMD_TRACE only; tools/dbg/trace_phases.py): lane 0 of every wave stamps the 100 MHz
// wall clock at tagged points into a [block][wave][256] table set with mmd_debug_set_trace().
#ifdef MMD_TRACE
__device__ unsigned long long* g_trace = nullptr;
#define TR(tag)                                                                                                       \
  do {                                                                                                                \
    if (g_trace && (threadIdx.x & 63) == 0)                                                                           \
      g_trace[((size_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 256 + (tag)] = wall_clock64();                          \
  } while (0)
#else
#define TR(tag) do { } while (0)
#endif

// The thread index through an opaque copy, for addresses that depend on nothing but the thread: inside the persistent kernel's step
// loop they are loop invariant, and hoisted out of the loop they were kept -- spilled to scratch -- across the whole forward (a
// reload waits for every weight load in flight).  Recomputing them where they are used costs a few VALU instructions.
__device__ __forceinline__ int opaque_tid() {
  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));
  return tid;
}
template <int CTRL>
__device__ __forceinline__ float dpp_add(float v) {   // v + v[DPP-permuted lane] in one VALU op
  return v + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
// ----------------------------------------------------------------------------------------------------------------
constexpr int MAX_IDENT = 3;

struct RtbPtrs {
  // Epilogue records (rec_load) of conv A / conv B per channel unit: bias, GroupNorm weight / bias, inverse per-channel weight scale of
  // the f16x2 pack (conv B: / act_a); a stage's first conv A: + the 1x1 residual conv's bias and inverse weight scale
  const float* ra; const float* rb;
  const float* tb;                          // conv A's time bias [C_out] (row t of the time table)
  const uint4* wa_bf; const uint4* wb_bf;   // f16x2 packs of the two convs
  float act_a;                              // static power-of-two scale of conv A's output activations = conv B's f16x2 input
};

struct ChainArgs {
  const float* in0;                      // [n, L, C0] network input (first chain only)
  RtbPtrs r0;
  const uint4* wa0_c1_bf;                // conv A pack of the second input chunk (up stages: cat(x, skip))
  const uint4* wres_bf;                  // f16x2 pack of the 1x1 residual conv (first input chunk)
  const uint4* wres_c1_bf;               // ... of the second input chunk (up stages)
  const uint4* wt_bf0; const uint4* wt_bf1;   // f16x2 pack(s) of the tail conv: Downsample1d, or the two parity passes of Upsample1d
  RtbPtrs ri[MAX_IDENT];
  const float* rt;                       // tail records (tail_rec): the tail conv's bias, the inverse channel scales of its pack(s)
  int n;
};

// The five stages, each an RTB with a 1x1 residual conv, identity RTBs and an optional strided / transposed tail conv; a workgroup owns
// the same 4 (2, 1) samples in every stage:
//   downs.0   4 -> 32 channels at L = 64: RTB, RTB, Downsample1d               (chain_body_d0w / d0s)
//   downs.1  32 -> 64 at L = 32: RTB, RTB (its output = skip1), Downsample1d   (chain_body_d1d)
//   downs.2 + mid_block1 / 2  64 -> 128 at L = 16: RTB + D2::N_IDENT RTBs      (chain_body_d2d)
//   ups.0    cat(x, skip2) 256 -> 64 at L = 16: RTB, RTB, Upsample1d           (chain_body_u0d)
//   ups.1    cat(x, skip1) 128 -> 32 at L = 32: RTB, RTB, Upsample1d, + the final block at L = 64   (chain_body_u1w / u1s)
// D2: downs.2 + mid blocks.  N_IDENT identity RTBs follow RTB 0, the skip tensor (skip2) is the output of RTB number MID_AFTER.
// XSTR / XSS: row and sample stride (floats) of the one row-form fp32 slab left, the stage's input as downs.1's tail hands it
// over: [sample][2 + position][channel], even row stride (two channels per 8-byte access), sample stride padded to 16 (mod 32)
// floats.  SLAB_OFF: the stage's Rd slab lies behind the x slab of the four samples.
struct D2 {
  static constexpr int N_IDENT = 3, MID_AFTER = 1, C0 = 64, XSTR = C0 + 2, SROWS = 16 + 4;
  static constexpr int XSS = SROWS * XSTR + (16 - (SROWS * XSTR) % 32 + 32) % 32;
  static constexpr int SLAB_OFF = (4 * XSS * 4 + 255) / 256 * 256;
  static_assert(N_IDENT <= MAX_IDENT && MID_AFTER >= 1, "ChainArgs::ri holds the identity RTBs");
};

constexpr int cmax(int a, int b) { return a > b ? a : b; }
// LDS of a workgroup: the largest stage is downs.2 / ups.0 -- the row-form fp32 x slab of downs.2's input + the 128-channel Rd
// slab (2 x 21504 B) behind it; downs.1 (input slab + 64-channel slab) and the four private slabs of the wave-private stages
// (downs.0, ups.1 + final block) fit below it (static_asserts at the stages: D0, U1, the stage bodies).
constexpr int MX_OFF = (D2::SLAB_OFF + 43008) / 4 + 8;
// + the per-sample maxima of the dynamic input scales + the second part of downs.2's lane-private residual parking area (the
// first part is the stage's dead x slab: 5 + 3 float4 per thread)
constexpr int PARK2_OFF = MX_OFF + MX_FLOATS;
constexpr int UNET_LDS_FLOATS = PARK2_OFF + 3 * 256 * 4;
static_assert(UNET_LDS_FLOATS * 4 == 76960, "LDS of a workgroup");

// GroupNorm-epilogue parameters of an RTB's conv A (with its time bias, tb_off floats into the table) / conv B for channels c0 ..
template <int NT>
__device__ __forceinline__ Epi<NT> epi_a(const RtbPtrs& R, int tb_off, int c0) { return epi_rec<NT>(R.ra, R.tb + tb_off, c0); }
template <int NT>
__device__ __forceinline__ Epi<NT> epi_b(const RtbPtrs& R, int c0) { return epi_rec<NT>(R.rb, nullptr, c0); }
// ... of a stage's first conv A, with the 1x1 residual conv's bias br and inverse weight scales isr from the same record
template <int NT>
__device__ __forceinline__ Epi<NT> epi_a_res(const RtbPtrs& R, int tb_off, int c0, float (&br)[NT], float (&isr)[NT]) {
  return epi_rec_res<NT>(R.ra, R.tb + tb_off, c0, br, isr);
}

// A weight pack in global memory as a wave reads it, n-tiles tile0 .. tile0 + NT - 1 (`frags` 1 KiB fragments [lane] x 16 B per n-tile): per
// n-tile a WAVE-UNIFORM base (pack + tile offset: tile0 comes from the wave index, so the whole address is the same in every lane and lives in
// a scalar register pair) + ONE 32-bit byte offset per lane, lane * 16, shared by all tiles and packs.  A fragment load is then
// global_load_dwordx4 v, vOff, s[base] offset:K; past the immediate's range the base moves on the scalar unit, which issues beside VALU and
// MFMA.  (As one 64-bit pointer per lane and tile the same loads cost two VGPRs per live pointer and a v_add_co / v_addc pair, with an s_nop
// for the VCC hazard between them, every two ring steps.)
typedef const __attribute__((address_space(1))) char* WBase;
__device__ __forceinline__ WBase wave_uniform_base(const void* p, unsigned byte_off) {
  const unsigned long long a = reinterpret_cast<unsigned long long>(p) + byte_off;
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a), hi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
  return (WBase)(((unsigned long long)hi << 32) | lo);
}
template <int NT> struct WTiles {
  WBase base[NT];
  unsigned off;
  // Fragment i of n-tile t (i is a constant wherever this is unrolled).  The load's immediate reaches -4 KiB .. +4 KiB - 1, i.e. eight
  // fragments around a base: the base moves in steps of 8 KiB (s_add_u32 / s_addc_u32), through an opaque copy -- left to itself the
  // compiler folds the constant behind the lane offset again, and then the whole address is a 64-bit VALU sum per lane.
  __device__ __forceinline__ u32x4 frag(int t, int i) const {
    const int adv = (i + 4) / 8 * 8192;
    unsigned long long b = reinterpret_cast<unsigned long long>(base[t]) + adv;
    if (adv) asm("" : "+s"(b));
    return *reinterpret_cast<const __attribute__((address_space(1))) u32x4*>((WBase)b + (i * 1024 - adv) + off);
  }
};
template <int NT>
__device__ __forceinline__ WTiles<NT> w_tiles(const void* w, int frags, int tile0, int lane) {
  WTiles<NT> r;
#pragma unroll
  for (int t = 0; t < NT; ++t) r.base[t] = wave_uniform_base(w, (unsigned)(tile0 + t) * (unsigned)frags * 1024u);
  r.off = (unsigned)lane * 16u;
  return r;
}
// The same view of a conv's pack staged in LDS (stage_weights: the half-sample stages), n-tiles 0 .. NT - 1: the lane's LDS pointers
template <int NT> struct WStaged {
  const u32x4* p[NT];
  __device__ __forceinline__ u32x4 frag(int t, int i) const { return p[t][i * 64]; }
};
template <int NT>
__device__ __forceinline__ WStaged<NT> w_staged(const char* wb, int frags, int lane) {
  WStaged<NT> r;
#pragma unroll
  for (int t = 0; t < NT; ++t) r.p[t] = reinterpret_cast<const u32x4*>(wb) + t * frags * 64 + lane;
  return r;
}
// fragment i of n-tile t of either view, or of plain per-tile lane pointers (tools/ubench)
template <int NT> __device__ __forceinline__ u32x4 w_frag(const WTiles<NT>& w, int t, int i) { return w.frag(t, i); }
template <int NT> __device__ __forceinline__ u32x4 w_frag(const WStaged<NT>& w, int t, int i) { return w.frag(t, i); }
__device__ __forceinline__ u32x4 w_frag(const u32x4* const* w, int t, int i) { return w[t][i * 64]; }
// A straight-line consumer's own copy of a view.  The scalar-base form of a load is selected only where the instruction selector sees the
// lane offset's zero-extension in the SAME basic block as the load; a lane offset that arrives from another block (a view built at the top
// of a stage, used behind a loop or a branch) has been widened there, and the address falls back to a 64-bit VALU sum per lane.  An opaque
// copy of the 32-bit offset at the consumer's entry (at most one v_mov_b32) pins the widening to the consumer's block.
template <int NT> __device__ __forceinline__ WTiles<NT> w_local(WTiles<NT> w) {
  asm volatile("" : "+v"(w.off));
  return w;
}
template <int NT> __device__ __forceinline__ WStaged<NT> w_local(const WStaged<NT>& w) { return w; }
__device__ __forceinline__ const u32x4* const* w_local(const u32x4* const* w) { return w; }
// ... of a second view read next to the first one (the residual conv's weights): it shares the first one's lane offset
template <int NT> __device__ __forceinline__ WTiles<NT> w_local(WTiles<NT> w, const WTiles<NT>& first) {
  w.off = first.off;
  return w;
}
template <class W, class F> __device__ __forceinline__ auto w_local(const W& w, const F&) { return w_local(w); }

// "Request the NEXT conv's first ring steps right behind this conv's taps", for a wave that holds `m_tiles` M tiles per conv.  At <= 2
// (unet_kernel<2> / <1>: the latency-bound launches of <= 512 trajectories, where nothing else on the CU covers an L2 round trip) they
// travel during the GroupNorm + Mish epilogue and the slab store instead of in front of the first MFMA (tools/ubench/pair_split.hip, arm
// basePF: 3 - 10 % of a conv); with four M tiles the ring registers would have to live through the epilogue of a 32-register tile.
constexpr bool ring_prefetch(int m_tiles) {
#ifdef MMD_NO_PF
  return false;                                              // (A/B side build: profiles/r06_prefetch_ab.txt)
#else
  return m_tiles <= 2;
#endif
}

// ---- tiles: t[M tile][n-tile] of f32x4 (a lane's 4 positions of one channel)
template <int M, int N>
__device__ __forceinline__ void tile_scale(f32x4 (&t)[M][N], float s) {
#pragma unroll
  for (int m = 0; m < M; ++m)
#pragma unroll
    for (int n = 0; n < N; ++n) t[m][n] *= s;
}
template <int M, int N>
__device__ __forceinline__ void tile_copy(f32x4 (&d)[M][N], const f32x4 (&s)[M][N]) {
#pragma unroll
  for (int m = 0; m < M; ++m)
#pragma unroll
    for (int n = 0; n < N; ++n) d[m][n] = s[m][n];
}
// the raw 1x1 residual conv -> the residual: times its weights' inverse scales and the input's inverse dynamic scale (of the S samples
// the M tiles belong to, M / S tiles each), + bias
template <int M, int N, int S>
__device__ __forceinline__ void tile_finish_res(f32x4 (&r)[M][N], const float (&isr)[N], const float (&inv)[S], const float (&br)[N]) {
#pragma unroll
  for (int m = 0; m < M; ++m)
#pragma unroll
    for (int n = 0; n < N; ++n) r[m][n] = r[m][n] * (isr[n] * inv[m / (M / S)]) + br[n];
}
template <int M, int N>
__device__ __forceinline__ void tile_finish_res(f32x4 (&r)[M][N], const float (&isr)[N], float inv, const float (&br)[N]) {
  const float inv1[1] = {inv};
  tile_finish_res(r, isr, inv1, br);
}
// tiles m0 .. m0 + MS - 1 of a larger tile
template <int MS, int M, int N>
__device__ __forceinline__ f32x4 (&sub_tile(f32x4 (&t)[M][N], int m0))[MS][N] { return reinterpret_cast<f32x4(&)[MS][N]>(t[m0]); }
template <int MS, int M, int N>
__device__ __forceinline__ const f32x4 (&sub_tile(const f32x4 (&t)[M][N], int m0))[MS][N] { return reinterpret_cast<const f32x4(&)[MS][N]>(t[m0]); }

// What a GroupNorm + Mish epilogue adds behind Mish.  Conv A of an RTB: the time bias, and the output is carried times act_s, the static
// f16x2 input scale of conv B (ACT); conv B: the residual tile.
template <int NT> struct AddTimeBias {
  static constexpr bool ACT = true;
  float tb[NT];
  ActScale as;
  __device__ __forceinline__ float operator()(int, int t, int) const { return tb[t]; }
};
template <int MT, int NT> struct AddResidual {
  static constexpr bool ACT = false;
  const f32x4 (&res)[MT][NT];
  ActScale as;
  __device__ __forceinline__ float operator()(int mt, int t, int r) const { return res[mt][t][r]; }
};
template <int NT>
__device__ __forceinline__ AddTimeBias<NT> gn_addend(const Epi<NT>& e, float act_s) {
  AddTimeBias<NT> a;
#pragma unroll
  for (int t = 0; t < NT; ++t) a.tb[t] = e.tb[t] * act_s;
  a.as = act_scale(act_s);
  return a;
}
template <int MT, int NT>
__device__ __forceinline__ AddResidual<MT, NT> gn_addend(const Epi<NT>&, const f32x4 (&res)[MT][NT]) { return AddResidual<MT, NT>{res, ActScale{}}; }

// sum over the CPG adjacent lanes (channels) of a GroupNorm group, same value in all of them
template <int CPG>
__device__ __forceinline__ float group_colsum(float v) {
  v = dpp_add<0xB1>(v);
  v = dpp_add<0x4E>(v);
  if constexpr (CPG >= 8) v = dpp_add<0x141>(v);
  if constexpr (CPG >= 16) v = dpp_add<0x140>(v);
  return v;
}


// ----------------------------------------------------------------------------------------------------------------
// DIRECT f16x2 convolutions on a row-form slab (downs.1, downs.2 + mid blocks, ups.0; the wave-private stages use the same
// GEMM loop on per-wave slabs).  Every weight fragment is re-used on 64 GEMM rows (a wave's unit is 1-2 n-tiles x the FOUR M
// tiles = samples of the workgroup), a conv is ONE slab store and one barrier pair, 8 accumulator streams (32-64 registers).
// (HISTORY.md section 3.1 has the history: the transform-domain forms of rounds 1-2 were bound by their weight stream.)
// GEMM: M tile s = sample s, row i = position; the taps of a k = 5 conv are row-shifted views of the slab
//     Rd[piece][lane group j][chunk kc][row = 20 s + 2 + position][8 channels]   (fp16, 2-row zero halo per sample)
// (channel block kc + KC j, KC = C / 32: the four blocks of a K = 32 chunk lie G = a multiple of 256 B apart, so a b128 A
// read is conflict free; the blocks of one lane group BX = 1280 + 32 B, so the epilogue's dword stores -- lanes = 4
// channel pairs x 4 blocks x 4 position groups -- are 2-way at worst, which is free).  C/D layout: a lane holds positions
// 4 g .. 4 g + 3 (g = lane >> 4) of ALL four samples for its 1-2 channels; a GroupNorm group (8 lanes x 16 positions) is
// reduced by three DPP steps and two cross-row shuffles.  Weights: per n-tile [tap][chunk kc][piece][lane] x 16 B.
// ----------------------------------------------------------------------------------------------------------------
template <int C> struct RdGeo {
  static constexpr int KC = C / 32, RPS = 20, BX = 4 * RPS * 16 + 32, G = (KC * BX + 255) / 256 * 256, PS = 4 * G, BYTES = 2 * PS;
  static constexpr int FRAGS5 = 5 * KC * 2;                  // weight fragments per n-tile of a k = 5 conv
  static constexpr int tile_row(int m) { return m * RPS; }   // first slab row (halo included) of M tile m = sample m
};
// The same slab for a stage of length 32 (downs.1): a sample is TWO M tiles (positions 0 .. 15, 16 .. 31) between its 2-row
// halos, 36 rows per sample; a wave's four M tiles are the two samples of its sample pair.
template <int C> struct RlGeo {
  static constexpr int KC = C / 32, RPS = 36, BX = 4 * RPS * 16 + 32, G = (KC * BX + 255) / 256 * 256, PS = 4 * G, BYTES = 2 * PS;
  static constexpr int FRAGS5 = 5 * KC * 2, FRAGS3 = 3 * KC * 2;
  static constexpr int tile_row(int m) { return (m >> 1) * RPS + (m & 1) * 16; }
};
template <class GEO>
__device__ __forceinline__ void rd_zero_halo(char* slab) {
  constexpr int TOT = N_PIECES * 4 * GEO::KC * 4 * 4;        // pieces x lane groups x chunks x samples x halo rows, 16 B each
  for (int idx = opaque_tid(); idx < TOT; idx += 256) {
    const int hr = idx & 3, sm = (idx >> 2) & 3, blk = (idx >> 4) % (4 * GEO::KC), q = idx / (64 * GEO::KC);
    *reinterpret_cast<uint4*>(slab + q * GEO::PS + (blk / GEO::KC) * GEO::G + (blk % GEO::KC) * GEO::BX +
                              (sm * GEO::RPS + (hr < 2 ? hr : GEO::RPS - 4 + hr)) * 16) = make_uint4(0u, 0u, 0u, 0u);
  }
}
template <class GEO, int NT, class W>
__device__ __forceinline__ void rd_load_b(u32x4 (&b)[NT][2], const W& w, int step) {   // W: anything w_frag reads
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int q = 0; q < 2; ++q) b[t][q] = w_frag(w, t, step * 2 + q);
}
// A fragments of one sample PAIR (M tiles 2 hp, 2 hp + 1; SM = 1: of the single M tile) at slab-row offset rowoff, chunk kc
template <class GEO, int SM = 2>
__device__ __forceinline__ void rd_load_a(u32x4 (&a)[SM][2], const char* va, int rowoff, int kc, int hp) {
#pragma unroll
  for (int sm = 0; sm < SM; ++sm)
#pragma unroll
    for (int q = 0; q < 2; ++q)
      a[sm][q] = *reinterpret_cast<const u32x4*>(va + q * GEO::PS + kc * GEO::BX + (GEO::tile_row(SM * hp + sm) + rowoff) * 16);
}
constexpr int RD_RD = 2;                    // weight ring depth in steps
#ifndef MMD_D2_RD
#define MMD_D2_RD 3
#endif
#ifndef MMD_D1_RD
#define MMD_D1_RD 3
#endif
#ifndef MMD_U0C_RD
#define MMD_U0C_RD 4
#endif
#ifndef MMD_U0_RD
#define MMD_U0_RD 3
#endif
template <class GEO, int NT, int RD = RD_RD, class W>
__device__ __forceinline__ void rd_ring_load(u32x4 (&b)[RD][NT][2], const W& w_in) {
  const auto w = w_local(w_in);
#pragma unroll
  for (int i = 0; i < RD; ++i) rd_load_b<GEO, NT>(b[i], w, i);
  MMD_PIN_LOADS();
}
// acc[sample][tile] (+)= conv over TAPS taps (slab rows TAP0 .. TAP0 + TAPS - 1 relative to the output position) x the C
// channels of the slab; va = slab + the lane's A offset (lane group lane >> 4, row lane & 15); w = the NT tiles' packs (WTiles /
// WStaged); b = ring pre-loaded with the first RD_RD steps.  RES: the stage's 1x1 residual conv rides on the centre tap's A
// fragments (res[sample][tile] (+)=, weights wr: per tile [chunk kc][piece]).  FRESH: start from zero.
template <class GEO, int NT, int TAP0, int TAPS, bool FRESH, bool RES, int MT = 4, int RD = RD_RD, class W, class WR>
__device__ __forceinline__ void rd_taps(f32x4 (&acc)[MT][NT], f32x4 (&res)[MT][NT], const char* va, const W& w_in, const WR& wr_in,
                                        u32x4 (&b)[RD][NT][2]) {
  const auto w = w_local(w_in);
  [[maybe_unused]] const auto wr = w_local(wr_in, w);
  // M tiles are processed in pairs (SM = 2), or a single one (MT = 1: the half-sample waves of unet_kernel<2> at L = 32)
  constexpr int KC = GEO::KC, STEPS = TAPS * KC, SM = MT >= 2 ? 2 : 1, HP = MT / SM;
  static_assert(MT == 1 || MT % 2 == 0, "M tiles are processed in pairs");
  // A fragments are double-buffered by M-tile pair (half a step = 2 M tiles x NT n-tiles x 3 MFMAs): 32 registers
  u32x4 a[2][SM][2];
  rd_load_a<GEO, SM>(a[0], va, TAP0, 0, 0);
  // (the residual conv's weights are requested RES_LOOK steps before the centre tap's step that uses them: loaded there,
  // every one of its steps would wait for an L2 round trip; all up front, they would cost 32 registers for two taps)
  constexpr int C0 = (2 - TAP0) * KC;                        // the centre tap's first step
  constexpr int RES_LOOK = C0 < 3 ? C0 : 3;
  u32x4 brp[RES ? KC : 1][NT][2];
  auto load_br = [&](int kc) {
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int q = 0; q < 2; ++q) brp[kc][t][q] = w_frag(wr, t, kc * 2 + q);
  };
  // Every step (tap, chunk kc) is unrolled: the ring slot step % RD and the A buffer parity are static for any depth, the
  // loop has no branches, and the scheduler sees the whole conv (rolled over the taps, downs.2's convs ran 5 % slower at <= 512
  // trajectories).
#pragma unroll
  for (int tap = 0; tap < TAPS; ++tap)
#pragma unroll
    for (int kc = 0; kc < KC; ++kc) {
      const int st = tap * KC + kc, ri = st % RD;
      const bool zero = FRESH && st == 0, last_kc = kc + 1 == KC, with_res = RES && TAP0 + tap == 2;
      if constexpr (RES) {
        if (st + RES_LOOK >= C0 && st + RES_LOOK < C0 + KC) load_br(st + RES_LOOK - C0);
      }
#pragma unroll
      for (int hp = 0; hp < HP; ++hp) {
        // the next half step's A fragments (the next M-tile pair; then the next chunk, or chunk 0 of the next tap; past the
        // last step: a valid, unused read)
        const int cur = (st * HP + hp) & 1;
        if (hp + 1 < HP) rd_load_a<GEO, SM>(a[cur ^ 1], va, TAP0 + tap, kc, hp + 1);
        else rd_load_a<GEO, SM>(a[cur ^ 1], va, last_kc ? TAP0 + tap + 1 : TAP0 + tap, last_kc ? 0 : kc + 1, 0);
        MMD_PIN_LOADS();
        const u32x4(&ac)[SM][2] = a[cur];
        const u32x4(&bc)[NT][2] = b[ri];
#pragma unroll
        for (int sm = 0; sm < SM; ++sm)
#pragma unroll
          for (int t = 0; t < NT; ++t) {
            if (zero) vb_three<true>(acc[SM * hp + sm][t], ac[sm], bc[t]);
            else vb_three<false>(acc[SM * hp + sm][t], ac[sm], bc[t]);
          }
        if constexpr (RES) {
          if (with_res) {
#pragma unroll
            for (int sm = 0; sm < SM; ++sm)
#pragma unroll
              for (int t = 0; t < NT; ++t) {
                const u32x4(&bw)[2] = brp[kc][t];
                if (FRESH && kc == 0) vb_three<true>(res[SM * hp + sm][t], ac[sm], bw);
                else vb_three<false>(res[SM * hp + sm][t], ac[sm], bw);
              }
          }
        }
      }
      if (st + RD < STEPS) rd_load_b<GEO, NT>(b[ri], w, st + RD);
      MMD_PIN_LOADS();
    }
}
// GroupNorm + Mish of the direct-layout tile acc[sample][tile] (raw f16x2 conv output: true value = acc * isc[tile] *
// inv[sample]) + add(sample, tile, r); NG = values per group (16 channels x 16 positions for two interleaved n-tiles at C =
// 128, 8 x 16 for one n-tile at C = 64); the lane's NT channels all belong to one group, which is 8 lanes x the wave's four
// 16-lane rows (position groups).
template <int NT, int NG, bool ACT, class ADD, int NS>
__device__ __forceinline__ void rd_gn_mish(f32x4 (&acc)[NS][NT], const float (&bias)[NT], const float (&gamma)[NT],
                                           const float (&beta)[NT], const float (&isc)[NT], const float (&inv)[NS],
                                           const ActScale& as, ADD add) {
  constexpr float inv_n = 1.f / (float)NG;
  float bsum = 0.f;
#pragma unroll
  for (int t = 0; t < NT; ++t) bsum += bias[t];
  const float bmean = group_colsum<8>(bsum) * 16.f * inv_n;
  float k[NS][NT], sum[NS], dm[NS][NT], sq[NS];
#pragma unroll
  for (int sm = 0; sm < NS; ++sm) {
    float v = 0.f;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      k[sm][t] = isc[t] * inv[sm];
      v = fmaf((acc[sm][t][0] + acc[sm][t][1]) + (acc[sm][t][2] + acc[sm][t][3]), k[sm][t], v);
    }
    sum[sm] = group_colsum<8>(v);
  }
#pragma unroll
  for (int sm = 0; sm < NS; ++sm) sum[sm] = add_xor16(sum[sm]);
#pragma unroll
  for (int sm = 0; sm < NS; ++sm) sum[sm] = add_xor32(sum[sm]);
#pragma unroll
  for (int sm = 0; sm < NS; ++sm) {
    const float mean = fmaf(sum[sm], inv_n, bmean);
    float v = 0.f;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      dm[sm][t] = mean - bias[t];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float d = fmaf(acc[sm][t][r], k[sm][t], -dm[sm][t]);
        v = fmaf(d, d, v);
      }
    }
    sq[sm] = group_colsum<8>(v);
  }
#pragma unroll
  for (int sm = 0; sm < NS; ++sm) sq[sm] = add_xor16(sq[sm]);
#pragma unroll
  for (int sm = 0; sm < NS; ++sm) sq[sm] = add_xor32(sq[sm]);
#pragma unroll
  for (int sm = 0; sm < NS; ++sm) {
    const float rstd = __builtin_amdgcn_rsqf(fmaf(sq[sm], inv_n, 1e-5f));   // (argument >= 1e-5: no denormal handling needed)
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      GnCoef cf = gn_coef(dm[sm][t], rstd, gamma[t], beta[t]);
      cf.sa *= k[sm][t];
#pragma unroll
      for (int r = 0; r < 4; r += 2) {
        const f32x2_t o = gn_mish2<ACT>(f32x2_t{acc[sm][t][r], acc[sm][t][r + 1]}, cf, f32x2_t{add(sm, t, r), add(sm, t, r + 1)}, as);
        acc[sm][t][r] = o.x;
        acc[sm][t][r + 1] = o.y;
      }
    }
  }
}
// The epilogue of a conv of the workgroup-slab stages.  `addend`: conv A's act_s (+ the time bias, output carried times act_s) or conv
// B's residual tile (gn_addend)
template <int NG, int NS, int NT, class ADDEND>
__device__ __forceinline__ void rd_gn(f32x4 (&acc)[NS][NT], const Epi<NT>& e, const float (&inv)[NS], const ADDEND& addend) {
  const auto add = gn_addend(e, addend);
  rd_gn_mish<NT, NG, decltype(add)::ACT>(acc, e.b, e.g, e.be, e.is, inv, add.as, add);
}
// per-sample |x| maxima of a direct-layout tile -> mx region 0 (and region2 if > 0): row_max16, one cross-row step,
// lanes 0 / 32 write the wave's two partials: slots 2 wave + {0, 1} of MX_SLOTS = 8
template <int NT, int NS>
__device__ __forceinline__ void rd_dyn_out(const f32x4 (&acc)[NS][NT], float* mx, int wave, int lane, int region2) {
#pragma unroll
  for (int sm = 0; sm < NS; ++sm) {
    float m = 0.f;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) m = fmaxf(m, fabsf(acc[sm][t][r]));
    m = row_max16(m);
    m = max_xor16(m);
    if ((lane & 31) == 0) {
      mx[sm * MX_SLOTS + 2 * wave + (lane >> 5)] = m;
      if (region2) mx[region2 * MX_REGION + sm * MX_SLOTS + 2 * wave + (lane >> 5)] = m;
    }
  }
}
__device__ __forceinline__ float mx_read(const float* mx, int sm) {
  const float4 p = *reinterpret_cast<const float4*>(mx + sm * MX_SLOTS), q = *reinterpret_cast<const float4*>(mx + sm * MX_SLOTS + 4);
  // (every slot holds a maximum of absolute values, written by rd_dyn_out / pair_maxima_out / half_sample_max / the tails: >= 0)
  return max_nn(max_nn(max_nn(p.x, p.y), max_nn(p.z, p.w)), max_nn(max_nn(q.x, q.y), max_nn(q.z, q.w)));
}
// dynamic input scale of a conv on tile t (samples s0 .. s0 + S - 1, M / S M tiles each) from the samples' maxima in mx: scale in place;
// inv: the inverse scales
template <int M, int N, int S>
__device__ __forceinline__ void mx_scale_tile(const float* mx, int s0, f32x4 (&t)[M][N], float (&inv)[S]) {
#pragma unroll
  for (int sl = 0; sl < S; ++sl) {
    const DynScale ds = dyn_scale(mx_read(mx, s0 + sl));
    inv[sl] = ds.inv;
    tile_scale(sub_tile<M / S>(t, M / S * sl), ds.s);
  }
}
// two-interleaved-n-tile tile (lane: channels c0, c0 + 1 = block 4 wave + (n >> 2), dword n & 3; positions 4 g + r) -> slab
template <class GEO, int NS>
__device__ __forceinline__ void rd_store2(char* vs, const f32x4 (&acc)[NS][2]) {   // vs = slab + lane's (block, row 2 + 4 g, dword)
#pragma unroll
  for (int sm = 0; sm < NS; ++sm)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const F16Pair f = f16_split2(acc[sm][0][r], acc[sm][1][r]);
      *reinterpret_cast<unsigned*>(vs + (sm * GEO::RPS + r) * 16) = f.hi;
      MMD_LO(*reinterpret_cast<unsigned*>(vs + GEO::PS + (sm * GEO::RPS + r) * 16) = f.lo;)
    }
}
// one-n-tile tile (lane: channel c, positions 4 g + r of the NS samples): the lanes of a pair (n, n ^ 1) swap half the samples,
// the even lane stores the first NS / 2 samples of channels (c, c + 1), the odd lane the other half of (c - 1, c).
// vs = slab + the lane's (block of c, row 2 + 4 g, dword (c & 7) >> 1) offset
template <class GEO, int NS>
__device__ __forceinline__ void rd_store1(char* vs, const f32x4 (&acc)[NS][1], int lane) {
  constexpr int HS = NS / 2;
  const bool odd = lane & 1;
  if constexpr (NS == 1) {
    // one sample: BOTH lanes of a pair store the same dword (c, c + 1) -- no divergent branch around the store: with the store under
    // `if (even lane)` the results were wrong on the hardware (the cross-lane read apparently ends up inside the branch, where the odd
    // lanes are disabled and read as 0); the duplicate same-value LDS write is free
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float own = acc[0][0][r];
      const float recv = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, own), 0xB1, 0xf, 0xf, true));
      const F16Pair f = f16_split2(odd ? recv : own, odd ? own : recv);        // (low channel, high channel)
      *reinterpret_cast<unsigned*>(vs + r * 16) = f.hi;
      MMD_LO(*reinterpret_cast<unsigned*>(vs + GEO::PS + r * 16) = f.lo;)
    }
  }
#pragma unroll
  for (int h = 0; h < HS; ++h)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float send = odd ? acc[h][0][r] : acc[HS + h][0][r];
      const float recv = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, send), 0xB1, 0xf, 0xf, true));
      const float own = odd ? acc[HS + h][0][r] : acc[h][0][r];
      const F16Pair f = f16_split2(odd ? recv : own, odd ? own : recv);        // (low channel, high channel)
      char* p = vs + ((odd ? HS + h : h) * GEO::RPS + r) * 16;
      *reinterpret_cast<unsigned*>(p) = f.hi;
      MMD_LO(*reinterpret_cast<unsigned*>(p + GEO::PS) = f.lo;)
    }
}
// row-form fp32 slab [sample][20][XSTR] (2-row halo) of C channels -> the Rd slab, times the sample's dynamic scale
template <int C, int XSS, int XSTR, int NS>
__device__ __forceinline__ void rowform_to_rd(const float* xslab, char* slab, const float* mx) {
  using GEO = RdGeo<C>;
  constexpr int CP2 = C / 2, ITEMS = 16 * NS * CP2;          // (sample, position) x channel pairs
  static_assert(ITEMS % 256 == 0 && XSTR % 2 == 0, "items per thread; 8-byte aligned channel pairs");
  const int tid = opaque_tid();
#pragma unroll
  for (int it = 0; it < ITEMS / 256; ++it) {
    const int idx = it * 256 + tid;
    const int cp = idx % CP2, sp = idx / CP2, sm = sp >> 4, pos = sp & 15;
    const float sc = dyn_scale(mx_read(mx, sm)).s;
    const float2 t = *reinterpret_cast<const float2*>(xslab + sm * XSS + (2 + pos) * XSTR + 2 * cp);
    const F16Pair f = f16_split2(t.x * sc, t.y * sc);
    const int blk = cp >> 2;
    char* dst = slab + (blk / GEO::KC) * GEO::G + (blk % GEO::KC) * GEO::BX + (sm * GEO::RPS + 2 + pos) * 16 + (cp & 3) * 4;
    *reinterpret_cast<unsigned*>(dst) = f.hi;
    MMD_LO(*reinterpret_cast<unsigned*>(dst + GEO::PS) = f.lo;)
  }
}

// ----------------------------------------------------------------------------------------------------------------
// WAVE-PRIVATE direct stages (downs.0; one sample per wave): at L = 64 a sample is four M tiles of its own, and with 32
// channels a wave holds a whole sample (4 M tiles x 2 interleaved n-tiles = 8 accumulators) -- so every conv of the stage
// reads only what the same wave wrote: no workgroup barrier anywhere inside the stage (LDS operations of one wave execute in
// order), GroupNorm statistics and the dynamic input scales are wave reductions, and the weights (20 KB per conv) are
// streamed by each wave.  Slab of one sample: Rw[piece][lane group j][chunk kc][row = 2 + position][8 channels].
// ----------------------------------------------------------------------------------------------------------------
template <int C, int L> struct RwGeo {
  static constexpr int KC = C / 32, RPS = 16, ROWS = L + 4, BX = ROWS * 16 + 32, G = (KC * BX + 255) / 256 * 256, PS = 4 * G;
  static constexpr int BYTES = 2 * PS, FRAGS5 = 5 * KC * 2, FRAGS3 = 3 * KC * 2;
  static constexpr int tile_row(int m) { return m * RPS; }   // M tile m = positions 16 m .. 16 m + 15 of the wave's sample
};
// A slab read at STRIDE 2 (Downsample1d = a k3 conv at the even positions only): M tile m = outputs 16 m .. 16 m + 15 of a
// sample = slab rows 2 (16 m + n) + tap of it, so the lane offset in `va` is n x 32 B (the caller adds n x 16 to the stride-1
// va) and the 16 lanes of a row group span 512 B: the b128 reads are 2-way bank conflicts, half as many of them and half the
// MFMAs and weight loads of the conv evaluated at every position.  SROWS = slab rows from one sample to the next.
template <class GEO, int SROWS, int TILES_PER_SAMPLE> struct Stride2 : GEO {
  static constexpr int tile_row(int m) { return (m / TILES_PER_SAMPLE) * SROWS + (m % TILES_PER_SAMPLE) * 32; }
};
__device__ __forceinline__ float wave_sum_rows(float v) {   // v + the same lane of the other three 16-lane rows
  v = add_xor16(v);
  v = add_xor32(v);
  return v;
}
template <int GL>
__device__ __forceinline__ float rw_gsum(float v) {          // sum over the GL lanes of a group and the wave's four 16-lane rows
  v = dpp_add<0xB1>(v);
  if constexpr (GL >= 4) v = dpp_add<0x4E>(v);
  if constexpr (GL >= 8) v = dpp_add<0x141>(v);
  return wave_sum_rows(v);
}
// GroupNorm + Mish of ONE sample's tile acc[M tile][tile] (positions 16 mt + 4 g + r; true value = acc * isc[tile] * inv);
// GL = lanes per group (the lane's NT channels belong to one group), NG = values per group
template <int MT, int NT, int GL, int NG, bool ACT, class ADD>
__device__ __forceinline__ void rw_gn_mish(f32x4 (&acc)[MT][NT], const float (&bias)[NT], const float (&gamma)[NT],
                                           const float (&beta)[NT], const float (&isc)[NT], float inv, const ActScale& as, ADD add) {
  constexpr float inv_n = 1.f / (float)NG;
  float k[NT], bsum = 0.f, v = 0.f;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    k[t] = isc[t] * inv;
    bsum += bias[t];
    float st = 0.f;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) st += (acc[mt][t][0] + acc[mt][t][1]) + (acc[mt][t][2] + acc[mt][t][3]);
    v = fmaf(st, k[t], v);
  }
  // mean over the group of (x + bias): every channel's bias counts at the sample's 16 MT positions, 4 per lane row
  const float mean = (rw_gsum<GL>(v) + rw_gsum<GL>(bsum) * (float)(4 * MT)) * inv_n;
  float dm[NT], q = 0.f;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    dm[t] = mean - bias[t];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float d = fmaf(acc[mt][t][r], k[t], -dm[t]);
        q = fmaf(d, d, q);
      }
  }
  const float rstd = __builtin_amdgcn_rsqf(fmaf(rw_gsum<GL>(q), inv_n, 1e-5f));
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    GnCoef cf = gn_coef(dm[t], rstd, gamma[t], beta[t]);
    cf.sa *= k[t];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int r = 0; r < 4; r += 2) {
        const f32x2_t o = gn_mish2<ACT>(f32x2_t{acc[mt][t][r], acc[mt][t][r + 1]}, cf, f32x2_t{add(mt, t, r), add(mt, t, r + 1)}, as);
        acc[mt][t][r] = o.x;
        acc[mt][t][r + 1] = o.y;
      }
  }
}
// The same for the stages whose waves are whole samples in unet_kernel<4> and HALF samples in unet_kernel<2> (downs.0, ups.1 +
// final block): the statistics of a sample are DEFINED through its two halves (positions [0, L / 2) and [L / 2, L): HT = 1 or 2
// M tiles each) -- per half the mean of x = acc k + bias over the group and the sum of squared deviations from THAT mean, combined
// by the pairwise update mean = (m0 + m1) / 2, M2 = (M2_0 + M2_1) + (m1 - m0)^2 N / 4.  A whole-sample wave evaluates both halves
// itself; two half-sample waves evaluate one each and swap (mean, M2) through LDS -- the same arithmetic, the same bits.
struct HalfStat { float mean, m2; };
// bsum4 = rw_gsum(sum of the lane's biases) (every channel's bias counts once per position: 4 positions per lane row and M tile)
template <int HT, int NT, int GL, int NG>
__device__ __forceinline__ HalfStat rw_half_stat(const f32x4 (&acc)[HT][NT], const float (&bias)[NT], const float (&k)[NT], float bsum4) {
  float v = 0.f;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    float st = (acc[0][t][0] + acc[0][t][1]) + (acc[0][t][2] + acc[0][t][3]);
    if constexpr (HT == 2) st += (acc[1][t][0] + acc[1][t][1]) + (acc[1][t][2] + acc[1][t][3]);
    v = fmaf(st, k[t], v);
  }
  HalfStat h;
  h.mean = (rw_gsum<GL>(v) + bsum4 * (float)(4 * HT)) * (2.f / (float)NG);
  float q = 0.f;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const float dm = h.mean - bias[t];
#pragma unroll
    for (int mt = 0; mt < HT; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float d = fmaf(acc[mt][t][r], k[t], -dm);
        q = fmaf(d, d, q);
      }
  }
  h.m2 = rw_gsum<GL>(q);
  return h;
}
struct GnStat { float mean, rstd; };
template <int NG>
__device__ __forceinline__ GnStat gn_combine(const HalfStat& h0, const HalfStat& h1) {
  const float dlt = h1.mean - h0.mean;
  const float m2 = fmaf(dlt * dlt, 0.25f * (float)NG, h0.m2 + h1.m2);
  return GnStat{0.5f * (h0.mean + h1.mean), __builtin_amdgcn_rsqf(fmaf(m2, 1.f / (float)NG, 1e-5f))};
}
// GroupNorm affine + Mish + add(mt, t, r) on MT tiles with the sample's statistics st
template <int MT, int NT, bool ACT, class ADD>
__device__ __forceinline__ void rw_gn_apply(f32x4 (&acc)[MT][NT], const float (&bias)[NT], const float (&gamma)[NT],
                                            const float (&beta)[NT], const float (&k)[NT], const GnStat& st, const ActScale& as, ADD add) {
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    GnCoef cf = gn_coef(st.mean - bias[t], st.rstd, gamma[t], beta[t]);
    cf.sa *= k[t];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int r = 0; r < 4; r += 2) {
        const f32x2_t o = gn_mish2<ACT>(f32x2_t{acc[mt][t][r], acc[mt][t][r + 1]}, cf, f32x2_t{add(mt, t, r), add(mt, t, r + 1)}, as);
        acc[mt][t][r] = o.x;
        acc[mt][t][r + 1] = o.y;
      }
  }
}
// k[tile] = the factor from acc to the true value; returns bsum4 of rw_half_stat
template <int GL, int NT>
__device__ __forceinline__ float rw_gn_prologue(const float (&bias)[NT], const float (&isc)[NT], float inv, float (&k)[NT]) {
  float bsum = 0.f;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    k[t] = isc[t] * inv;
    bsum += bias[t];
  }
  return rw_gsum<GL>(bsum);
}
// ... of a WHOLE sample held by one wave (MT = 2 HT M tiles)
template <int MT, int NT, int GL, int NG, bool ACT, class ADD>
__device__ __forceinline__ void rw_gn_mish_whole(f32x4 (&acc)[MT][NT], const float (&bias)[NT], const float (&gamma)[NT],
                                                 const float (&beta)[NT], const float (&isc)[NT], float inv, const ActScale& as, ADD add) {
  constexpr int HT = MT / 2;
  static_assert(MT == 2 || MT == 4, "two halves of one or two M tiles");
  float k[NT];
  const float bsum4 = rw_gn_prologue<GL>(bias, isc, inv, k);
  const HalfStat h0 = rw_half_stat<HT, NT, GL, NG>(sub_tile<HT>(acc, 0), bias, k, bsum4);
  const HalfStat h1 = rw_half_stat<HT, NT, GL, NG>(sub_tile<HT>(acc, HT), bias, k, bsum4);
  rw_gn_apply<MT, NT, ACT>(acc, bias, gamma, beta, k, gn_combine<NG>(h0, h1), as, add);
}
// ... of the HALF sample this wave holds (HT M tiles; half index hf); the partner wave's statistics arrive through xch = the
// sample's exchange area [2 halves][64 lanes] of HalfStat (one workgroup barrier; the caller guarantees another barrier between
// this read and the next write of the area)
template <int HT, int NT, int GL, int NG, bool ACT, class ADD>
__device__ __forceinline__ void rw_gn_mish_half(f32x4 (&acc)[HT][NT], const float (&bias)[NT], const float (&gamma)[NT],
                                                const float (&beta)[NT], const float (&isc)[NT], float inv, const ActScale& as, ADD add,
                                                HalfStat* xch, int hf, int lane) {
  float k[NT];
  const float bsum4 = rw_gn_prologue<GL>(bias, isc, inv, k);
  const HalfStat own = rw_half_stat<HT, NT, GL, NG>(acc, bias, k, bsum4);
  xch[hf * 64 + lane] = own;
  __syncthreads();
  const HalfStat other = xch[(hf ^ 1) * 64 + lane];
  const GnStat st = hf ? gn_combine<NG>(other, own) : gn_combine<NG>(own, other);
  rw_gn_apply<HT, NT, ACT>(acc, bias, gamma, beta, k, st, as, add);
}
template <int MT, int NT>
__device__ __forceinline__ float rw_absmax(const f32x4 (&acc)[MT][NT]) {   // the sample's |x| maximum, in every lane
  float m = 0.f;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) m = fmaxf(m, fabsf(acc[mt][t][r]));
  return wave_max(m);
}
// two-interleaved-n-tile tile of one sample (lane: channels 2 n, 2 n + 1 (+ 32 per further pair); positions 16 mt + 4 g + r)
// -> the wave's slab; vs = slab + the lane's (block n >> 2, row 2 + 4 g, dword n & 3) offset
template <class GEO, int MT>
__device__ __forceinline__ void rw_store2(char* vs, const f32x4 (&acc)[MT][2]) {
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const F16Pair f = f16_split2(acc[mt][0][r], acc[mt][1][r]);
      *reinterpret_cast<unsigned*>(vs + (mt * 16 + r) * 16) = f.hi;
      MMD_LO(*reinterpret_cast<unsigned*>(vs + GEO::PS + (mt * 16 + r) * 16) = f.lo;)
    }
}
__device__ __forceinline__ void wave_lds_fence() {           // a wave's own LDS writes before its own later reads
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// The epilogue of a conv of the wave-private stages, on the wave's whole sample or (RwHalf) on its half of the sample.  `addend`: as rd_gn
struct RwHalf { HalfStat* xch; int hf, lane; };              // the partner-wave exchange of rw_gn_mish_half
template <int GL, int NG, int MT, int NT, class ADDEND>
__device__ __forceinline__ void rw_gn(f32x4 (&acc)[MT][NT], const Epi<NT>& e, float inv, const ADDEND& addend) {
  const auto add = gn_addend(e, addend);
  rw_gn_mish_whole<MT, NT, GL, NG, decltype(add)::ACT>(acc, e.b, e.g, e.be, e.is, inv, add.as, add);
}
template <int GL, int NG, int HT, int NT, class ADDEND>
__device__ __forceinline__ void rw_gn(f32x4 (&acc)[HT][NT], const Epi<NT>& e, float inv, const ADDEND& addend, const RwHalf& h) {
  const auto add = gn_addend(e, addend);
  rw_gn_mish_half<HT, NT, GL, NG, decltype(add)::ACT>(acc, e.b, e.g, e.be, e.is, inv, add.as, add, h.xch, h.hf, h.lane);
}
// ... on downs.1's tile of S samples x M / S M tiles, sample by sample (a sample's group is wave-internal there: rw_gn_mish)
template <int TPS>
__device__ __forceinline__ float sample_of(float act_s, int) { return act_s; }
template <int TPS, int M, int N>
__device__ __forceinline__ const f32x4 (&sample_of(const f32x4 (&t)[M][N], int sl))[TPS][N] { return sub_tile<TPS>(t, TPS * sl); }
template <int GL, int NG, int M, int NT, int S, class ADDEND>
__device__ __forceinline__ void rw_gn_samples(f32x4 (&acc)[M][NT], const Epi<NT>& e, const float (&inv)[S], const ADDEND& addend) {
  constexpr int TPS = M / S;
#pragma unroll
  for (int sl = 0; sl < S; ++sl) {
    const auto add = gn_addend(e, sample_of<TPS>(addend, sl));
    rw_gn_mish<TPS, NT, GL, NG, decltype(add)::ACT>(sub_tile<TPS>(acc, TPS * sl), e.b, e.g, e.be, e.is, inv[sl], add.as, add);
  }
}
// Zero the four halo rows (0, 1, rows + 2, rows + 3) of a wave-private-geometry slab: 4 KC blocks x N_PIECES pieces, one 16-byte store
// per lane (KC = 1, two pieces: lanes 0 .. 31).  base = the slab's first row; `mine`: whether this wave is the one that zeroes (half-sample stages: one
// wave per sample)
template <class GEO>
__device__ __forceinline__ void rw_zero_halo(char* base, int rows, int lane, bool mine) {
  constexpr int KC = GEO::KC;
  if (mine && (16 * N_PIECES * KC >= 64 || lane < 16 * N_PIECES * KC)) {
    const int hr = lane & 3, blk = (lane >> 2) % (4 * KC), q = lane / (16 * KC);
    *reinterpret_cast<uint4*>(base + q * GEO::PS + (blk / KC) * GEO::G + (blk % KC) * GEO::BX + (hr < 2 ? hr : rows + hr) * 16) =
        make_uint4(0u, 0u, 0u, 0u);
  }
}
// per-sample |x| maxima of a tile in downs.1's layout (wave = (channel half np = wave & 1, sample pair sp = wave >> 1); M tiles 2 sl,
// 2 sl + 1 = sample NS / 2 * sp + sl) -> K of the sample's mx slots from SLOT0 on (the two waves of a sample pair fill 2 K slots)
template <int K, int SLOT0, int NS>
__device__ __forceinline__ void pair_maxima_out(const f32x4 (&v)[NS][2], float* mx, int wave, int lane) {
  constexpr int SW = NS / 2;
  const int np = wave & 1, s0 = SW * (wave >> 1);
  float m2[2] = {0.f, 0.f};
#pragma unroll
  for (int sl = 0; sl < SW; ++sl) m2[sl] = rw_absmax(sub_tile<2>(v, 2 * sl));
  if (lane < K * SW) mx[(s0 + lane / K) * MX_SLOTS + SLOT0 + np + 2 * (lane & (K - 1))] = SW == 2 && lane / K ? m2[1] : m2[0];
}
// strided tail: y = y * is + bt in place; returns the wave's |y| maximum
template <int MT, int NT>
__device__ __forceinline__ float tail_epilogue(f32x4 (&y)[MT][NT], const float (&is)[NT], const float (&bt)[NT]) {
  float m = 0.f;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        y[mt][t][r] = fmaf(y[mt][t][r], is[t], bt[t]);
        m = fmaxf(m, fabsf(y[mt][t][r]));
      }
  return wave_max(m);
}
// transposed tail: the same for its two parity passes e / o (even / odd output positions); the maximum over both
template <int MT, int NT>
__device__ __forceinline__ float tail_up_epilogue(f32x4 (&e)[MT][NT], f32x4 (&o)[MT][NT], const float (&is0)[NT], const float (&is1)[NT],
                                                  const float (&bt)[NT]) {
  float m = 0.f;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        e[mt][t][r] = fmaf(e[mt][t][r], is0[t], bt[t]);
        o[mt][t][r] = fmaf(o[mt][t][r], is1[t], bt[t]);
        m = fmaxf(m, fmaxf(fabsf(e[mt][t][r]), fabsf(o[mt][t][r])));
      }
  return wave_max(m);
}

// Cooperative weight staging of the half-sample stages (unet_kernel<2>): there every wave of the workgroup needs ALL B fragments of
// a 32 -> 32 conv, and four waves fetching the same 20 KB through the CU's 64 B/clk vector-memory path took ~0.8 us per conv
// (the issue of the loads itself blocks: profiles/r04_trace_512_half_sample.txt).  Instead the conv's NFRAG fragments (1 KiB
// each: [lane] x 16 B, contiguous in the pack) go global -> LDS ONCE per workgroup by LDS-DMA (global_load_lds_dwordx4: no
// registers; wave w moves fragments w, w + 4, ...), one conv ahead into the other of two buffers, and the GEMM loop reads its B
// fragments from LDS through a two-step ring.  The issuing wave waits for its own pieces (vmcnt) before the barrier that
// publishes the slab the conv reads.
template <int NFRAG>
__device__ __forceinline__ void stage_weights(const uint4* w, char* dst, int wave, int lane) {
  static_assert(NFRAG % 4 == 0, "fragments are dealt to the four waves");
  const uint4* src = w + lane;
  if constexpr (N_PIECES == 2) {
#pragma unroll
    for (int i = 0; i < NFRAG / 4; ++i) {
      const int f = wave + 4 * i;
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + f * 64),
                                       (__attribute__((address_space(3))) void*)(dst + f * 1024), 16, 0, 0);
    }
  } else {
    // one piece: the fragments alternate piece 0 / piece 1 ([tap][chunk][piece], an even count per n-tile), only the even ones are
    // moved, dealt to the four waves (the wave index is uniform: a scalar branch on the ragged last round)
    constexpr int NF0 = NFRAG / 2;
#pragma unroll
    for (int i = 0; i < (NF0 + 3) / 4; ++i) {
      const int f = 2 * (wave + 4 * i);
      if (4 * i + 3 < NF0 || wave + 4 * i < NF0)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + f * 64),
                                         (__attribute__((address_space(3))) void*)(dst + f * 1024), 16, 0, 0);
    }
  }
}
__device__ __forceinline__ void staged_weights_landed() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
constexpr int WBUF_BYTES = 20 * 1024;                        // the largest staged conv: 32 -> 32, k = 5, two pieces
// The half-sample stages (wave = (sample sp = wave >> 1, half hf = wave & 1)): the sample's maximum of a per-wave partial -- both waves
// publish theirs in the sample's mx slots (4 hf .. 4 hf + 3), barrier
__device__ __forceinline__ float half_sample_max(float* mx, int sp, int hf, int lane, float own) {
  if (lane < 4) mx[sp * MX_SLOTS + 4 * hf + lane] = own;
  __syncthreads();
  return mx_read(mx, sp);
}

// downs.0 (4 -> 32 -> 32 channels at L = 64, Downsample1d): wave = sample.  The first conv's K is 5 taps x 4 channels = 20
// of the 32 slots of ONE MFMA chunk (im2col: lane group j holds taps 2 j, 2 j + 1 -- two consecutive 8-byte rows of the
// [row][4 channel] input slab), its 1x1 residual conv a second chunk with only the centre tap's slots non-zero.  The raw
// network input has no bounded range: dynamic scale from the sample's own maximum.  The stride-2 tail reads its slab at stride 2
// (Stride2: 3 taps on two M tiles, 36 MFMAs; the A reads are 2-way bank conflicted, half as many as at every position).
// The stage's output goes straight into the next stage's input slab (RlGeo<32>) as f16 pieces under the sample's own dynamic
// scale, behind a workgroup barrier (it aliases the waves' slabs); the sample's maximum goes to mx.
//
// Two schedules: chain_body_d0w (wave = sample: unet_kernel<4>) and chain_body_d0s (wave = half a sample: unet_kernel<2> / <1>).  What
// defines values or layout is written once below, on MT M tiles from tile m0 of the sample on: a wave of d0w holds tiles 0 .. 3, a wave of
// d0s tiles 2 hf, 2 hf + 1 -- the same arithmetic, the same bits.
struct D0 {
  using GW = RwGeo<32, 64>;
  static constexpr int XIN = 72 * 8;                          // bytes per piece of the [row][4 channel] input slab (rows -2 .. 69)
  static constexpr int W_BYTES = GW::BYTES + 2 * XIN + 128;   // a sample's conv slab + input slab
  static_assert(4 * W_BYTES <= MX_OFF * 4, "four private slabs");
  static_assert(2 * W_BYTES + 2 * WBUF_BYTES <= MX_OFF * 4, "two samples' slabs + two weight buffers below the maxima");
  static_assert(GW::FRAGS5 * 2 * 1024 <= WBUF_BYTES, "a staged conv fits its buffer");
};
// Sample `smp` (`valid`: it exists, else zeros), lane = position: its dynamic scale from its own maximum, f16 pieces -> rows [2 +
// position][4 channels] of the input slab's two pieces where `store` (d0s: the wave's half).  Returns the inverse scale.
__device__ __forceinline__ float d0_stage_input(const float* in0, bool valid, size_t smp, int lane, char* xin, bool store) {
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (valid) v = *reinterpret_cast<const float4*>(in0 + (smp * 64 + lane) * 4);
  const DynScale ds = dyn_scale(wave_max(fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w)))));
  const F16Pair p0 = f16_split2(v.x * ds.s, v.y * ds.s), p1 = f16_split2(v.z * ds.s, v.w * ds.s);
  if (store) {
    *reinterpret_cast<uint2*>(xin + (2 + lane) * 8) = make_uint2(p0.hi, p1.hi);
    MMD_LO(*reinterpret_cast<uint2*>(xin + D0::XIN + (2 + lane) * 8) = make_uint2(p0.lo, p1.lo);)
  }
  return ds.inv;
}
__device__ __forceinline__ void d0_zero_xin_halo(char* xin, int lane, bool mine) {   // rows 0, 1, 66 .. 71 of both pieces
  if (mine && lane < 8 * N_PIECES) {
    const int row = (lane & 7) < 2 ? (lane & 7) : 64 + (lane & 7);
    *reinterpret_cast<uint2*>(xin + (lane >> 3) * D0::XIN + row * 8) = make_uint2(0u, 0u);
  }
}
// the B fragments of RTB 0's conv A (im2col chunk) and of the 1x1 residual conv: one chunk x two pieces per n-tile
__device__ __forceinline__ void d0_load_wa(const ChainArgs& a, int lane, u32x4 (&b)[2][2], u32x4 (&br)[2][2]) {
  const WTiles<2> wa = w_local(w_tiles<2>(a.r0.wa_bf, 2, 0, lane)), wr = w_local(w_tiles<2>(a.wres_bf, 2, 0, lane), wa);
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      b[t][q] = wa.frag(t, q);
      br[t][q] = wr.frag(t, q);
    }
}
// RTB 0's conv A + the 1x1 residual conv on M tiles m0 .. m0 + MT - 1
template <int MT>
__device__ __forceinline__ void d0_conv_a(f32x4 (&acc)[MT][2], f32x4 (&res)[MT][2], const char* xin, int m0, int n, int g,
                                          const u32x4 (&b)[2][2], const u32x4 (&br)[2][2]) {
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    u32x4 af[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const uint2* p = reinterpret_cast<const uint2*>(xin + q * D0::XIN + ((m0 + mt) * 16 + n + 2 * g) * 8);
      const uint2 lo = p[0], hi = p[1];
      af[q] = u32x4{lo.x, lo.y, hi.x, hi.y};
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      vb_three<true>(acc[mt][t], af, b[t]);
      vb_three<true>(res[mt][t], af, br[t]);
    }
  }
}
// The tail's output tiles m0 .. m0 + MT - 1 of sample `smp` (outputs q = 16 (m0 + mt) + 4 g + r) -> the next stage's input slab
// (RlGeo<32>: rows 36 sample + 2 + q), channels 2 n, 2 n + 1 = block n >> 2, dword n & 3, as f16 pieces under the sample's own
// dynamic scale `so` (the next stage reads it from mx)
template <int MT>
__device__ __forceinline__ void d0_tail_store(char* lb, int smp, int m0, int n, int g, const f32x4 (&y)[MT][2], float so) {
  using GN = RlGeo<32>;
  char* xb = lb + (n >> 2) * GN::G + (smp * GN::RPS + 2 + 16 * m0 + 4 * g) * 16 + (n & 3) * 4;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const F16Pair f = f16_split2(y[mt][0][r] * so, y[mt][1][r] * so);
      *reinterpret_cast<unsigned*>(xb + (16 * mt + r) * 16) = f.hi;
      MMD_LO(*reinterpret_cast<unsigned*>(xb + GN::PS + (16 * mt + r) * 16) = f.lo;)
    }
}

template <int NS>     // NS: the workgroup's samples (a wave >= NS runs on zeros and stores nothing)
__device__ __forceinline__ void chain_body_d0w(const ChainArgs& a, float* lds, int n0, int lane, int wave, int trb, int tb_off = 0) {
  using GW = D0::GW;
  char* const slab = reinterpret_cast<char*>(lds) + wave * D0::W_BYTES;
  char* const xin = slab + GW::BYTES;
  const int n = lane & 15, g = lane >> 4, c0 = 2 * n;
  const char* const va = slab + g * GW::G + n * 16;          // A fragment: row lane & 15, lane group lane >> 4 (KC = 1: block j)
  char* const vs = slab + (n >> 2) * GW::G + (2 + 4 * g) * 16 + (n & 3) * 4;
  TR(trb + 0);
  // ---- stage the sample, zero rows around it and the halo rows of the conv slab
  const float inv_in = d0_stage_input(a.in0, wave < NS && n0 + wave < a.n, n0 + wave, lane, xin, true);
  d0_zero_xin_halo(xin, lane, true);
  rw_zero_halo<GW>(slab, 64, lane, true);
  wave_lds_fence();
  f32x4 acc[4][2], res[4][2];
  float br0[2], isr0[2];
  const Epi<2> e0a = epi_a_res<2>(a.r0, tb_off, c0, br0, isr0);
  // ---- RTB 0 conv A (im2col chunk) + the 1x1 residual conv
  {
    u32x4 b[2][2], br[2][2];
    d0_load_wa(a, lane, b, br);
    d0_conv_a<4>(acc, res, xin, 0, n, g, b, br);
  }
  // The whole weight set of a conv (5 taps x 2 n-tiles x 2 pieces = 20 KB per wave) is requested BEFORE the epilogue that
  // produces the conv's input (preload), so the L2 latency hides behind GroupNorm + Mish instead of in front of the MFMAs.
  u32x4 ring[5][2][2];
  auto preload = [&](const uint4* w) { rd_ring_load<GW, 2, 5>(ring, w_tiles<2>(w, GW::FRAGS5, 0, lane)); };
  auto conv = [&](const uint4* w) {                          // one 32 -> 32 conv over the tile in acc (already scaled)
    const WTiles<2> wp = w_tiles<2>(w, GW::FRAGS5, 0, lane);
    rw_store2<GW, 4>(vs, acc);
    wave_lds_fence();
    rd_taps<GW, 2, 0, 5, true, false, 4, 5>(acc, res, va, wp, wp, ring);
    wave_lds_fence();                                        // (the next store must not overtake these reads)
  };
  tile_finish_res(res, isr0, inv_in, br0);
  preload(a.r0.wb_bf);
  rw_gn<2, 256>(acc, e0a, inv_in, a.r0.act_a);
  TR(trb + 1);
  {
    const Epi<2> e = epi_b<2>(a.r0, c0);
    conv(a.r0.wb_bf);
    preload(a.ri[0].wa_bf);
    rw_gn<2, 256>(acc, e, 1.f, res);
  }
  TR(trb + 2);
  // ---- identity RTB
  {
    const RtbPtrs& R = a.ri[0];
    tile_copy(res, acc);
    const DynScale ds = dyn_scale(rw_absmax(acc));
    tile_scale(acc, ds.s);
    const Epi<2> ea = epi_a<2>(R, tb_off, c0);
    conv(R.wa_bf);
    preload(R.wb_bf);
    rw_gn<2, 256>(acc, ea, ds.inv, R.act_a);
    TR(trb + 3);
    const Epi<2> eb = epi_b<2>(R, c0);
    conv(R.wb_bf);
    rw_gn<2, 256>(acc, eb, 1.f, res);
    TR(trb + 4);
  }
  // ---- tail: Downsample1d = Conv1d(k3, s2, p1): y[p] = sum_t x[p + t - 1] W_t at the even p
  {
    const DynScale ds = dyn_scale(rw_absmax(acc));
    tile_scale(acc, ds.s);
    const WTiles<2> wt = w_tiles<2>(a.wt_bf0, GW::FRAGS3, 0, lane);
    u32x4 ring3[3][2][2];
    const TailRec<2, 1> tl = tail_rec<2, 1>(a.rt, c0);
    const float ist[2] = {tl.is[0][0] * ds.inv, tl.is[0][1] * ds.inv};
    rd_ring_load<GW, 2, 3>(ring3, wt);
    rw_store2<GW, 4>(vs, acc);
    wave_lds_fence();
    // (outputs q = 16 mt + 4 g + r = the even positions 2 q: two M tiles read at stride 2)
    f32x4 y[2][2];
    rd_taps<Stride2<GW, 0, 2>, 2, 1, 3, true, false, 2, 3>(y, y, va + n * 16, wt, wt, ring3);
    const float mo = tail_epilogue(y, ist, tl.bt);
    __syncthreads();                                         // every wave is done with its slab: the next stage's slab aliases them
    if (lane < MX_SLOTS) (lds + MX_OFF)[wave * MX_SLOTS + lane] = mo;
    char* const lb = reinterpret_cast<char*>(lds);
    d0_tail_store<2>(lb, wave, 0, n, g, y, dyn_scale(mo).s);
    rw_zero_halo<RlGeo<32>>(lb + wave * RlGeo<32>::RPS * 16, 32, lane, true);   // (the sample's rows 0, 1, 34, 35)
  }
  TR(trb + 5);
}

// downs.0 for unet_kernel<2> (two trajectories per workgroup): a sample is split between two waves by POSITION -- wave = (sample sp =
// wave >> 1, half hf = wave & 1: positions 32 hf .. 32 hf + 31 = M tiles 2 hf, 2 hf + 1 of the sample's four), so all four waves
// work on real data with half the MFMAs and half the epilogue values each (the whole-sample form left two waves on zeros).  The
// two waves share the sample's slab (a conv's taps reach two rows into the other half: one workgroup barrier between the slab
// store and the taps), GroupNorm statistics are the two-half combination of rw_half_stat (one exchange through LDS per conv,
// whose barrier also orders the next slab store behind the partner's taps), dynamic scales take the sample's maximum from the
// two waves' partials in mx.  Weights come through LDS (stage_weights), one conv ahead, into two buffers behind the two samples' slabs.
template <int NV>     // NV: the workgroup's REAL samples (unet_kernel<1>: sample 1 is fed zeros and never stored)
__device__ __forceinline__ void chain_body_d0s(const ChainArgs& a, float* lds, int n0, int lane, int wave, int trb, int tb_off = 0) {
  using GW = D0::GW;
  const int sp = wave >> 1, hf = wave & 1;
  char* const slab = reinterpret_cast<char*>(lds) + sp * D0::W_BYTES;
  char* const xin = slab + GW::BYTES;
  float* const mx = lds + MX_OFF;
  const RwHalf half{reinterpret_cast<HalfStat*>(lds + PARK2_OFF) + sp * 128, hf, lane};   // (downs.2's parking area is idle in this stage)
  static_assert(2 * 128 * sizeof(HalfStat) <= 3 * 256 * 16, "exchange area inside the parking area");
  char* const wb0 = reinterpret_cast<char*>(lds) + 2 * D0::W_BYTES;
  char* const wb1 = wb0 + WBUF_BYTES;
  stage_weights<2 * GW::FRAGS5>(a.r0.wb_bf, wb0, wave, lane);     // RTB 0's conv B: lands while the sample is staged and conv A runs
  const int n = lane & 15, g = lane >> 4, c0 = 2 * n;
  const char* const va = slab + g * GW::G + (n + 32 * hf) * 16;
  char* const vs = slab + (n >> 2) * GW::G + (2 + 4 * g + 32 * hf) * 16 + (n & 3) * 4;
  TR(trb + 0);
  // ---- stage the sample: every wave loads all of it (lane = position: the exact maximum without an exchange) and writes its half
  const float inv_in = d0_stage_input(a.in0, sp < NV && n0 + sp < a.n, n0 + sp, lane, xin, (lane >> 5) == hf);
  d0_zero_xin_halo(xin, lane, hf == 0);
  rw_zero_halo<GW>(slab, 64, lane, hf == 0);
  f32x4 acc[2][2], res[2][2];
  float br0[2], isr0[2];
  const Epi<2> e0a = epi_a_res<2>(a.r0, tb_off, c0, br0, isr0);
  u32x4 b0[2][2], br[2][2];
  d0_load_wa(a, lane, b0, br);
  __syncthreads();
  // ---- RTB 0 conv A (im2col chunk) + the 1x1 residual conv on the half's two M tiles
  d0_conv_a<2>(acc, res, xin, 2 * hf, n, g, b0, br);
  u32x4 ring[2][2][2];
  // one 32 -> 32 conv over the half tile in acc (already scaled), its weights staged in wb; behind the barrier the NEXT conv's
  // NEXT_FRAGS fragments start on their way into the other buffer (every wave is past the conv that read it)
  auto conv = [&](char* wb, auto next_frags, const uint4* w_next, char* wb_next, int tr = -1) {
    const WStaged<2> wp = w_staged<2>(wb, GW::FRAGS5, lane);
    if (tr >= 0) TR(tr);
    rw_store2<GW, 2>(vs, acc);
    if (tr >= 0) TR(tr + 1);
    staged_weights_landed();
    __syncthreads();                                         // both halves of the sample and the conv's weights are in LDS
    if (tr >= 0) TR(tr + 2);
    if constexpr (decltype(next_frags)::value > 0) stage_weights<decltype(next_frags)::value>(w_next, wb_next, wave, lane);
    rd_ring_load<GW, 2, 2>(ring, wp);
    rd_taps<GW, 2, 0, 5, true, false, 2, 2>(acc, res, va, wp, wp, ring);
    if (tr >= 0) TR(tr + 3);
  };
  using F5 = std::integral_constant<int, 2 * GW::FRAGS5>;
  using F3 = std::integral_constant<int, 2 * GW::FRAGS3>;
  tile_finish_res(res, isr0, inv_in, br0);
  rw_gn<2, 256>(acc, e0a, inv_in, a.r0.act_a, half);
  TR(trb + 1);
  {
    const Epi<2> e = epi_b<2>(a.r0, c0);
    conv(wb0, F5{}, a.ri[0].wa_bf, wb1);
    rw_gn<2, 256>(acc, e, 1.f, res, half);
  }
  TR(trb + 2);
  // ---- identity RTB
  {
    const RtbPtrs& R = a.ri[0];
    tile_copy(res, acc);
    const DynScale ds = dyn_scale(half_sample_max(mx, sp, hf, lane, rw_absmax(acc)));
    tile_scale(acc, ds.s);
    const Epi<2> ea = epi_a<2>(R, tb_off, c0);
    conv(wb1, F5{}, R.wb_bf, wb0, trb + 6);
    TR(trb + 10);
    rw_gn<2, 256>(acc, ea, ds.inv, R.act_a, half);
    TR(trb + 3);
    const Epi<2> eb = epi_b<2>(R, c0);
    conv(wb0, F3{}, a.wt_bf0, wb1);
    rw_gn<2, 256>(acc, eb, 1.f, res, half);
    TR(trb + 4);
  }
  // ---- tail: Downsample1d = Conv1d(k3, s2, p1) at the even positions: the half's 16 outputs = ONE M tile read at stride 2
  {
    const DynScale ds = dyn_scale(half_sample_max(mx, sp, hf, lane, rw_absmax(acc)));
    tile_scale(acc, ds.s);
    const WStaged<2> wt = w_staged<2>(wb1, GW::FRAGS3, lane);
    const TailRec<2, 1> tl = tail_rec<2, 1>(a.rt, c0);
    const float ist[2] = {tl.is[0][0] * ds.inv, tl.is[0][1] * ds.inv};
    rw_store2<GW, 2>(vs, acc);
    staged_weights_landed();
    __syncthreads();
    f32x4 y[1][2];
    rd_ring_load<GW, 2, 2>(ring, wt);
    rd_taps<Stride2<GW, 0, 2>, 2, 1, 3, true, false, 1, 2>(y, y, va + n * 16, wt, wt, ring);
    const float mo = tail_epilogue(y, ist, tl.bt);
    // (the barrier inside: every wave is done with its slab -- the next stage's slab aliases them -- and the sample's maxima
    // are published for the next stage's dynamic scale)
    const float so = dyn_scale(half_sample_max(mx, sp, hf, lane, mo)).s;
    char* const lb = reinterpret_cast<char*>(lds);
    d0_tail_store<1>(lb, sp, hf, n, g, y, so);
    rw_zero_halo<RlGeo<32>>(lb + sp * RlGeo<32>::RPS * 16, 32, lane, hf == 0);   // (the sample's rows 0, 1, 34, 35)
  }
  TR(trb + 5);
}

// downs.1 (32 -> 64 -> 64 channels at L = 32, Downsample1d) in the direct form on RlGeo slabs.  Wave w = (n-tile pair np = w &
// 1: channels 32 np + 2 n + t, interleaved columns; sample pair sp = w >> 1: samples 2 sp, 2 sp + 1), so a weight fragment is
// used on four M tiles and fetched by two waves; acc[m][t]: M tile m = sample 2 sp + (m >> 1), positions 16 (m & 1) + 4 g + r.
// A GroupNorm group (8 channels x 32 positions of a sample) is 4 lanes x 2 tiles x the sample's 2 M tiles: wave-internal.
// The input slab arrives from downs.0's tail (f16 pieces, per-sample scales in mx); the strided tail reads its slab at stride 2
// (Stride2) and writes downs.2's row-form fp32 x slab (D2 geometry) + the per-sample maxima to mx.
// skip: the stage's skip tensor (output of its second RTB) in the acc layout.
template <int NS>
__device__ __forceinline__ void chain_body_d1d(const ChainArgs& a, float* lds, int lane, int wave, f32x4 (&skip)[NS][2], int trb, int tb_off = 0) {
  using GI = RlGeo<32>;
  using GH = RlGeo<64>;
  constexpr int H_OFF = GI::BYTES;                           // the 64-channel slab lies behind the input slab
  static_assert(H_OFF + GH::BYTES <= MX_OFF * 4, "input slab + 64-channel slab");
  char* const lb = reinterpret_cast<char*>(lds);
  char* const slabH = lb + H_OFF;
  float* const mx = lds + MX_OFF;
  // SW samples per wave: the pair 2 sp, 2 sp + 1 of a four-sample workgroup, or sample sp of a two-sample one (unet_kernel<2>: all
  // four waves on real samples, half the M tiles each); a sample = 2 M tiles, so a wave has NS of them
  constexpr int SW = NS / 2;
  const int n = lane & 15, g = lane >> 4, np = wave & 1, sp = wave >> 1, s0 = SW * sp;
  const int c0 = 32 * np + 2 * n;
  const char* const vaI = lb + g * GI::G + (s0 * GI::RPS + n) * 16;
  const char* const vaH = slabH + g * GH::G + (s0 * GH::RPS + n) * 16;
  // the lane's channel pair (c0, c0 + 1) = block 4 np + (n >> 2) = (chunk (n >> 2) & 1, lane group 2 np + (n >> 3)), dword n & 3
  char* const vsH = slabH + (2 * np + (n >> 3)) * GH::G + ((n >> 2) & 1) * GH::BX + (s0 * GH::RPS + 2 + 4 * g) * 16 + (n & 3) * 4;
  auto wt2 = [&](const uint4* w, int frags) { return w_tiles<2>(w, frags, 2 * np, lane); };
  f32x4 acc[NS][2], res[NS][2];
  constexpr int RD1 = MMD_D1_RD;                               // weight ring depth of the 64 -> 64 convs
  u32x4 ring[RD1][2][2];
  auto store_tile = [&]() {
#pragma unroll
    for (int m = 0; m < NS; ++m)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const F16Pair f = f16_split2(acc[m][0][r], acc[m][1][r]);
        *reinterpret_cast<unsigned*>(vsH + (GH::tile_row(m) + r) * 16) = f.hi;
        MMD_LO(*reinterpret_cast<unsigned*>(vsH + GH::PS + (GH::tile_row(m) + r) * 16) = f.lo;)
      }
  };
  // one 64 -> 64 conv over the tile in acc (already scaled); on entry every wave is past its reads of the slab.  PF (ring_prefetch: one
  // sample per wave = unet_kernel<2>): the NEXT conv's first ring steps are requested right behind this conv's taps and travel during
  // the epilogue; `frags_next`: the next pack's fragments per n-tile.
  constexpr bool PF = ring_prefetch(NS);
  auto prefetch = [&](const uint4* w, int frags) {
    if constexpr (PF) rd_ring_load<GH, 2, RD1>(ring, wt2(w, frags));
  };
  auto conv = [&](const uint4* w, const uint4* w_next, int frags_next) {
    const WTiles<2> wp = wt2(w, GH::FRAGS5);
    if constexpr (!PF) rd_ring_load<GH, 2, RD1>(ring, wp);
    store_tile();
    __syncthreads();
    rd_taps<GH, 2, 0, 5, true, false, NS, RD1>(acc, acc, vaH, wp, wp, ring);
    prefetch(w_next, frags_next);
  };
  float one2[SW];
#pragma unroll
  for (int sl = 0; sl < SW; ++sl) one2[sl] = 1.f;

  // =================== RTB 0 (32 -> 64): conv A + the 1x1 residual conv on the centre tap ===================
  {
    u32x4 ring5[5][2][2];
    const WTiles<2> wpa = wt2(a.r0.wa_bf, GI::FRAGS5), wpr = wt2(a.wres_bf, 2 * GI::KC);
    rd_ring_load<GI, 2, 5>(ring5, wpa);
    float br[2], isr[2];
    const Epi<2> e0a = epi_a_res<2>(a.r0, tb_off, c0, br, isr);
    __syncthreads();                                         // downs.0's tail has written the input slab and its maxima
    TR(trb + 0);
    float inv_in[SW];
#pragma unroll
    for (int sl = 0; sl < SW; ++sl) inv_in[sl] = dyn_scale(mx_read(mx, s0 + sl)).inv;
    rd_zero_halo<GH>(slabH);
    rd_taps<GI, 2, 0, 5, true, true, NS, 5>(acc, res, vaI, wpa, wpr, ring5);
    tile_finish_res(res, isr, inv_in, br);
    prefetch(a.r0.wb_bf, GH::FRAGS5);
    rw_gn_samples<4, 256>(acc, e0a, inv_in, a.r0.act_a);
  }
  TR(trb + 1);
  {
    const Epi<2> e = epi_b<2>(a.r0, c0);
    conv(a.r0.wb_bf, a.ri[0].wa_bf, GH::FRAGS5);             // (its slab is not the one conv A reads: no barrier before the store)
    rw_gn_samples<4, 256>(acc, e, one2, res);
  }
  TR(trb + 2);
  // =================== identity RTB ===================
  {
    const RtbPtrs& R = a.ri[0];
    tile_copy(res, acc);
    pair_maxima_out<4, 0>(acc, mx, wave, lane);              // (all eight slots of the wave's samples)
    __syncthreads();                                         // the previous conv is done reading the slab
    float inv[SW];
    mx_scale_tile(mx, s0, acc, inv);
    const Epi<2> ea = epi_a<2>(R, tb_off, c0);
    conv(R.wa_bf, R.wb_bf, GH::FRAGS5);
    rw_gn_samples<4, 256>(acc, ea, inv, R.act_a);
    TR(trb + 3);
    __syncthreads();
    const Epi<2> eb = epi_b<2>(R, c0);
    conv(R.wb_bf, a.wt_bf0, GH::FRAGS3);                     // (next: the strided tail's 3-tap pack)
    rw_gn_samples<4, 256>(acc, eb, one2, res);
    TR(trb + 4);
    tile_copy(skip, acc);
  }
  // =================== tail: Downsample1d = Conv1d(k3, s2, p1): y[p] = sum_t x[p + t - 1] W_t at the even p ===================
  {
    pair_maxima_out<4, 0>(acc, mx, wave, lane);
    __syncthreads();
    float inv[SW];
    mx_scale_tile(mx, s0, acc, inv);
    const WTiles<2> wt = wt2(a.wt_bf0, GH::FRAGS3);
    const TailRec<2, 1> tl = tail_rec<2, 1>(a.rt, c0);
    if constexpr (!PF) rd_ring_load<GH, 2, RD1>(ring, wt);
    store_tile();
    __syncthreads();
    // (outputs q = 4 g + r = the even positions 2 q of the wave's samples: one M tile each, read at stride 2; the GEMM loop takes
    // M tiles in pairs: a one-sample wave computes its tile twice)
    f32x4 y[2][2];
    rd_taps<Stride2<GH, SW == 2 ? GH::RPS : 0, 1>, 2, 1, 3, true, false, 2, RD1>(y, y, vaH + n * 16, wt, wt, ring);
    float m2[2] = {0.f, 0.f};
#pragma unroll
    for (int sl = 0; sl < SW; ++sl) {
      const float is[2] = {tl.is[0][0] * inv[sl], tl.is[0][1] * inv[sl]};
      m2[sl] = tail_epilogue(sub_tile<1>(y, sl), is, tl.bt);
    }
    __syncthreads();                                         // every wave is done reading the slab the next stage's x slab aliases
    if (lane < 4 * SW) mx[(s0 + (lane >> 2)) * MX_SLOTS + np + 2 * (lane & 3)] = (lane >> 2) ? m2[1] : m2[0];
    // -> the next stage's row-form fp32 x slab [sample][2 + q][D2::XSTR]
    float* xb = lds + s0 * D2::XSS + (2 + 4 * g) * D2::XSTR + c0;
#pragma unroll
    for (int sl = 0; sl < SW; ++sl)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        *reinterpret_cast<float2*>(xb + sl * D2::XSS + r * D2::XSTR) = make_float2(y[sl][0][r], y[sl][1][r]);
  }
  TR(trb + 5);
}

// downs.2 + mid blocks in the direct form.  Wave w owns the n-tiles 2 w, 2 w + 1 with INTERLEAVED columns (column n of tile h =
// channel 32 w + 2 n + h: adjacent channels per lane, dword slab stores) x all four samples; acc[sample][h][r] = position
// 4 (lane >> 4) + r.  acc: the stage's output; mid: the skip tensor (after RTB D2::MID_AFTER).
// Lane-private parking of a 32-register tile in LDS ([i][thread] x 16 B: conflict-free b128, no synchronisation -- a thread
// reads back only what it wrote): the residual tile of an RTB waits there instead of in 32 VGPRs while the block's two convs
// run (the kernel sits at the 256-register limit of two waves per SIMD; a compiler spill to scratch costs a vmcnt(0) wait
// behind every weight load in flight).  Parts 0 .. 4 in the stage's dead x slab, 5 .. 7 behind the maxima.
__device__ __forceinline__ float* park_slot(float* lds, int i) {
  return (i < 5 ? lds + i * 1024 : lds + PARK2_OFF + (i - 5) * 1024) + opaque_tid() * 4;
}
template <int NS>
__device__ __forceinline__ void park_tile(float* lds, const f32x4 (&t)[NS][2]) {
#pragma unroll
  for (int i = 0; i < 2 * NS; ++i) *reinterpret_cast<f32x4*>(park_slot(lds, i)) = t[i >> 1][i & 1];
}
template <int NS>
__device__ __forceinline__ void unpark_tile(float* lds, f32x4 (&t)[NS][2]) {
#pragma unroll
  for (int i = 0; i < 2 * NS; ++i) t[i >> 1][i & 1] = *reinterpret_cast<const f32x4*>(park_slot(lds, i));
}

template <int NS>
__device__ __forceinline__ void chain_body_d2d(const ChainArgs& a, float* lds, int lane, int wave, f32x4 (&acc)[NS][2],
                                               f32x4 (&mid)[NS][2], int trb, int tb_off = 0) {
  using G128 = RdGeo<128>;
  using G64 = RdGeo<64>;
  const int n = lane & 15, g = lane >> 4;
  const int c0 = 32 * wave + 2 * n;                          // the lane's channels c0 (tile 0), c0 + 1 (tile 1)
  // LDS: the row-form fp32 x slab (previous stage's tail tile) at the start, the Rd slab behind it (conv A's 64-channel
  // input uses its first bytes in the 64-channel geometry)
  static_assert(D2::SLAB_OFF + G128::BYTES <= MX_OFF * 4, "x slab + Rd slab must fit below the maxima");
  static_assert(D2::SLAB_OFF >= 5 * 1024 * 4, "the dead x slab holds 5 of the 8 parked float4 per thread");
  char* const slab = reinterpret_cast<char*>(lds) + D2::SLAB_OFF;
  float* const mx = lds + MX_OFF;
  const char* const va128 = slab + g * G128::G + n * 16;     // A fragment: row lane & 15 = position, lane group lane >> 4
  const char* const va64 = slab + g * G64::G + n * 16;
  char* const vs = slab + wave * G128::G + (n >> 2) * G128::BX + (2 + 4 * g) * 16 + (n & 3) * 4;
  auto wt2 = [&](const uint4* w, int frags) { return w_tiles<2>(w, frags, 2 * wave, lane); };
  constexpr int RDD = MMD_D2_RD;                               // weight ring depth of the 128 -> 128 convs
  u32x4 ring[RDD][2][2];
  const WTiles<2> wpa = wt2(a.r0.wa_bf, G64::FRAGS5), wpr = wt2(a.wres_bf, 2 * G64::KC);
  rd_ring_load<G64, 2, 2>(reinterpret_cast<u32x4(&)[2][2][2]>(ring), wpa);   // (conv A + residual streams: depth 2, or it spills)
  __syncthreads();                                           // the x slab (previous stage's tail tile) and its maxima are staged
  TR(trb + 0);

  float one4[NS];
#pragma unroll
  for (int sm = 0; sm < NS; ++sm) one4[sm] = 1.f;
  // conv B's epilogue: the residual tile comes back from its parking area
  auto gn_unparked = [&](const Epi<2>& e) {
    f32x4 res[NS][2];
    unpark_tile(lds, res);
    rd_gn<256>(acc, e, one4, res);
  };
  // one 128 -> 128 conv over the tile in acc (already scaled for f16x2); on entry every wave is past its reads of the slab.
  // PF (ring_prefetch): the first RDD weight steps of the NEXT conv are requested right behind this conv's taps.
  constexpr bool PF = ring_prefetch(NS);
  auto prefetch = [&](const uint4* w) {
    if constexpr (PF) rd_ring_load<G128, 2, RDD>(ring, wt2(w, G128::FRAGS5));
  };
  auto conv = [&](const uint4* w, const uint4* w_next) {
    const WTiles<2> wp = wt2(w, G128::FRAGS5);
    TR(trb + 10);
    if constexpr (!PF) rd_ring_load<G128, 2, RDD>(ring, wp);
    rd_store2<G128>(vs, acc);
    TR(trb + 11);
    __syncthreads();
    TR(trb + 12);
    rd_taps<G128, 2, 0, 5, true, false, NS, RDD>(acc, acc, va128, wp, wp, ring);
    if (w_next) prefetch(w_next);
    TR(trb + 13);
  };

  // =================== RTB 0 (64 -> 128): conv A + the 1x1 residual conv from the row-form x slab ===================
  float inv_in[NS];
#pragma unroll
  for (int sm = 0; sm < NS; ++sm) inv_in[sm] = dyn_scale(mx_read(mx, sm)).inv;
  rd_zero_halo<G64>(slab);
  float br[2], isr[2];
  const Epi<2> e0a = epi_a_res<2>(a.r0, tb_off, c0, br, isr);
  rowform_to_rd<D2::C0, D2::XSS, D2::XSTR, NS>(lds, slab, mx);
  __syncthreads();
  {
    f32x4 res[NS][2];
    rd_taps<G64, 2, 0, 5, true, true, NS, 2>(acc, res, va64, wpa, wpr, reinterpret_cast<u32x4(&)[2][2][2]>(ring));
    tile_finish_res(res, isr, inv_in, br);
    park_tile(lds, res);                                     // (every wave is past the barrier behind the x slab's last read)
  }
  prefetch(a.r0.wb_bf);                                      // (the 64 -> 128 conv's depth-2 ring is consumed: RTB 0's conv B travels now)
  rd_gn<256>(acc, e0a, inv_in, a.r0.act_a);
  TR(trb + 1);
  __syncthreads();                                           // conv A is done reading the 64-channel slab
  rd_zero_halo<G128>(slab);
  {
    const Epi<2> e = epi_b<2>(a.r0, c0);
    conv(a.r0.wb_bf, D2::N_IDENT > 0 ? a.ri[0].wa_bf : nullptr);
    gn_unparked(e);
  }

  // =================== identity RTBs ===================
#pragma unroll 1
  for (int k = 0; k < D2::N_IDENT; ++k) {
    const RtbPtrs& R = a.ri[k];
    park_tile(lds, acc);                                     // the block's input = its residual
    rd_dyn_out<2>(acc, mx, wave, lane, k == D2::MID_AFTER ? 1 : 0);   // (the input of the RTB after MID_AFTER is the skip tensor)
    __syncthreads();                                         // the previous conv is done reading the slab
    float inv[NS];
    mx_scale_tile(mx, 0, acc, inv);
    const Epi<2> ea = epi_a<2>(R, tb_off, c0);
    conv(R.wa_bf, R.wb_bf);
    rd_gn<256>(acc, ea, inv, R.act_a);
    __syncthreads();
    const Epi<2> eb = epi_b<2>(R, c0);
    conv(R.wb_bf, k + 1 < D2::N_IDENT ? a.ri[k + 1].wa_bf : nullptr);
    gn_unparked(eb);
    TR(trb + 18);
    if (D2::MID_AFTER == k + 1) tile_copy(mid, acc);
  }
  rd_dyn_out<2>(acc, mx, wave, lane, 2);                     // the stage's output: ups.0's conv A takes its maximum from region 2
}

// ups.0 in the direct form: cat(mid output, skip2) -> RTB (256 -> 64, with its 1x1 residual conv) -> RTB (64 -> 64) ->
// Upsample1d = ConvTranspose1d(k4, s2, p1) as two 2-tap parity passes, all f16x2 on Rd slabs.  Wave w owns the n-tile of
// channels 16 w + (lane & 15) x all four samples.  x0 / x1: the two 128-channel chunks of the input (downs.2's tiles, in
// ITS layout: store2(tile) writes one into the 128-channel slab); xe / xo: the stage's output (even / odd positions).
template <int NS, class STORE2>
__device__ __forceinline__ void chain_body_u0d(const ChainArgs& a, float* lds, int lane, int wave, f32x4 (&x0)[NS][2],
                                               f32x4 (&x1)[NS][2], STORE2 store2, char* slab128, f32x4 (&xe)[NS][1],
                                               f32x4 (&xo)[NS][1], int trb, int tb_off = 0) {
  using G128 = RdGeo<128>;
  using G64 = RdGeo<64>;
  const int n = lane & 15, g = lane >> 4, col = 16 * wave + n;
  char* const slab64 = reinterpret_cast<char*>(lds);
  static_assert(G64::BYTES <= MX_OFF * 4, "64-channel Rd slab");
  float* const mx = lds + MX_OFF;
  const char* const va128 = slab128 + g * G128::G + n * 16;
  const char* const va64 = slab64 + g * G64::G + n * 16;
  char* const vs64 = slab64 + wave * G64::G + (n >> 3) * G64::BX + (2 + 4 * g) * 16 + ((n & 7) >> 1) * 4;
  auto wt1 = [&](const uint4* w, int frags) { return w_tiles<1>(w, frags, wave, lane); };
  constexpr int RDU = MMD_U0_RD;                               // weight ring depth of conv A's two 128-channel chunks
  u32x4 ringa[RDU][1][2];
  constexpr int RDC = MMD_U0C_RD;                              // ... of the 64 -> 64 convs and the tail's parity passes
  u32x4 ring[RDC][1][2];
  const WTiles<1> wp0 = wt1(a.r0.wa_bf, G128::FRAGS5), wp1 = wt1(a.wa0_c1_bf, G128::FRAGS5);
  const WTiles<1> wr0 = wt1(a.wres_bf, 2 * G128::KC), wr1 = wt1(a.wres_c1_bf, 2 * G128::KC);
  rd_ring_load<G128, 1, RDU>(ringa, wp0);
  __syncthreads();                                           // the previous stage is done with the slab; its maxima are in mx
  TR(trb + 0);

  f32x4 acc[NS][1], res[NS][1];
  float one4[NS];
#pragma unroll
  for (int sm = 0; sm < NS; ++sm) one4[sm] = 1.f;
  // one 64 -> 64 conv over the tile in acc (already scaled); on entry every wave is past its reads of the slab.  PF (ring_prefetch): the
  // NEXT pack's first ring steps are requested right behind this conv's taps; `frags_next`: the next pack's fragments per n-tile.
  constexpr bool PF = ring_prefetch(NS);
  auto prefetch64 = [&](const uint4* w, int frags) {
    if constexpr (PF) rd_ring_load<G64, 1, RDC>(ring, wt1(w, frags));
  };
  auto conv64 = [&](const uint4* w, const uint4* w_next, int frags_next) {
    const WTiles<1> wp = wt1(w, G64::FRAGS5);
    if constexpr (!PF) rd_ring_load<G64, 1, RDC>(ring, wp);
    rd_store1<G64>(vs64, acc, lane);
    __syncthreads();
    rd_taps<G64, 1, 0, 5, true, false, NS, RDC>(acc, res, va64, wp, wp, ring);
    prefetch64(w_next, frags_next);
  };

  // =================== RTB 0: cat(x0, x1) -> 64 channels; the 1x1 residual conv rides on the centre tap ===================
  float inv_in[NS];
#pragma unroll
  for (int sm = 0; sm < NS; ++sm) {
    // residual-stream input: dynamic scale from the maxima downs.2 left in regions 1 (skip2) and 2 (mid output) of mx
    // (mx_read returns a maximum of absolute values: >= 0)
    const DynScale ds = dyn_scale(max_nn(mx_read(mx + MX_REGION, sm), mx_read(mx + 2 * MX_REGION, sm)));
    inv_in[sm] = ds.inv;
    tile_scale(sub_tile<1>(x0, sm), ds.s);
    tile_scale(sub_tile<1>(x1, sm), ds.s);
  }
  float br[1], isr[1];
  const Epi<1> e0a = epi_a_res<1>(a.r0, tb_off, col, br, isr);
  store2(x0);
  TR(160);
  __syncthreads();
  TR(161);
  rd_taps<G128, 1, 0, 5, true, true, NS, RDU>(acc, res, va128, wp0, wr0, ringa);
  rd_ring_load<G128, 1, RDU>(ringa, wp1);
  TR(162);
  __syncthreads();                                           // every wave is done reading chunk 0
  store2(x1);
  TR(163);
  __syncthreads();
  TR(164);
  rd_taps<G128, 1, 0, 5, false, true, NS, RDU>(acc, res, va128, wp1, wr1, ringa);
  TR(165);
  tile_finish_res(res, isr, inv_in, br);
  prefetch64(a.r0.wb_bf, G64::FRAGS5);
  rd_gn<128>(acc, e0a, inv_in, a.r0.act_a);
  TR(trb + 1);
  __syncthreads();                                           // chunk 1 is consumed
  rd_zero_halo<G64>(slab64);
  {
    const Epi<1> e = epi_b<1>(a.r0, col);
    conv64(a.r0.wb_bf, a.ri[0].wa_bf, G64::FRAGS5);
    rd_gn<128>(acc, e, one4, res);
  }
  TR(trb + 4);
  // =================== identity RTB ===================
  {
    const RtbPtrs& R = a.ri[0];
    tile_copy(res, acc);
    rd_dyn_out<1>(acc, mx, wave, lane, 0);
    __syncthreads();                                         // the previous conv is done reading the slab
    float inv[NS];
    mx_scale_tile(mx, 0, acc, inv);
    const Epi<1> ea = epi_a<1>(R, tb_off, col);
    conv64(R.wa_bf, R.wb_bf, G64::FRAGS5);
    rd_gn<128>(acc, ea, inv, R.act_a);
    TR(trb + 5);
    __syncthreads();
    const Epi<1> eb = epi_b<1>(R, col);
    conv64(R.wb_bf, a.wt_bf0, 2 * G64::KC * 2);              // (next: the transposed tail's first parity pack)
    rd_gn<128>(acc, eb, one4, res);
    TR(trb + 6);
  }
  // =================== tail: out[2 m] = in[m - 1] W3 + in[m] W1, out[2 m + 1] = in[m] W2 + in[m + 1] W0 ===================
  {
    rd_dyn_out<1>(acc, mx, wave, lane, 0);
    __syncthreads();
    float inv[NS];
    mx_scale_tile(mx, 0, acc, inv);
    const WTiles<1> wt0 = wt1(a.wt_bf0, 2 * G64::KC * 2), wt1p = wt1(a.wt_bf1, 2 * G64::KC * 2);
    const TailRec<1, 2> tl = tail_rec<1, 2>(a.rt, col);
    if constexpr (!PF) rd_ring_load<G64, 1, RDC>(ring, wt0);
    rd_store1<G64>(vs64, acc, lane);
    __syncthreads();
    TR(trb + 7);
    rd_taps<G64, 1, 1, 2, true, false, NS, RDC>(xe, res, va64, wt0, wt0, ring);
    rd_ring_load<G64, 1, RDC>(ring, wt1p);
    rd_taps<G64, 1, 2, 2, true, false, NS, RDC>(xo, res, va64, wt1p, wt1p, ring);
    // the stage's output stays in registers: xe / xo[sample][0][r] = positions 2 m, 2 m + 1 (m = 4 g + r) of channel col; the
    // per-sample maxima of the wave's 16 channels go to slot `wave` of mx region 0 (the caller's barrier publishes them)
#pragma unroll
    for (int sm = 0; sm < NS; ++sm) {
      const float s0[1] = {tl.is[0][0] * inv[sm]}, s1[1] = {tl.is[1][0] * inv[sm]};
      const float m = tail_up_epilogue(sub_tile<1>(xe, sm), sub_tile<1>(xo, sm), s0, s1, tl.bt);
      if (lane == 0) mx[sm * MX_SLOTS + wave] = m;
    }
  }
}

// ups.1 (cat(x, skip1): 128 -> 32 -> 32 channels at L = 32, Upsample1d) + the final block (Conv1dBlock 32 -> 32 at L = 64, 1x1
// conv 32 -> 4), wave = sample, all convs direct f16x2 (layers.py:346-358, temporal_unet.py:104-110, 166-172).  Only the
// first conv needs the other waves: its input arrives distributed by CHANNEL (ups.0's output xe / xo and the skip tensor kept
// from downs.1: wave w holds channels 16 w + (lane & 15) of all four samples), so the two 64-channel chunks are written into
// the four samples' slabs across waves, one after the other through the same 10 KB slab (4 workgroup barriers); everything
// after it -- 3 convs, the transposed tail as two parity passes, the final block and the output store -- reads only what the
// same wave wrote (wave_lds_fence).  Slabs: RwGeo<64, 32> (conv A chunks), RwGeo<32, 32>, RwGeo<32, 64> (final block).
//
// Two schedules, as for downs.0: chain_body_u1w (wave = sample) and chain_body_u1s (wave = half a sample); the fragments below define
// values and layout for both, on MT M tiles from tile m0 of the sample on.
struct U1 {
  using GA = RwGeo<64, 32>;
  using GB = RwGeo<32, 32>;
  using GF = RwGeo<32, 64>;
  static constexpr int W_BYTES = cmax(GA::BYTES, cmax(GB::BYTES, GF::BYTES)) + 128;   // a sample's slab
  static constexpr int RDA = 5;                               // conv A's weight ring: half a chunk ahead
  static constexpr int TF = 2 * (2 * GB::KC * 2);             // fragments of one parity pass of the transposed tail (both n-tiles)
  static_assert(4 * W_BYTES <= MX_OFF * 4, "four private slabs");
  static_assert(2 * W_BYTES + 2 * WBUF_BYTES <= MX_OFF * 4, "two samples' slabs + two weight buffers below the maxima");
  static_assert(GB::FRAGS5 * 2 * 1024 <= WBUF_BYTES && GF::FRAGS5 * 2 * 1024 <= WBUF_BYTES, "a staged conv fits its buffer");
};
__device__ __forceinline__ float lane_swap1(float v) {       // the value of the partner lane (n ^ 1)
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xf, 0xf, true));
}
// The dynamic input scales of conv A from the maxima in mx region 0 (slots 0 .. 3: ups.0's output, 4 .. 7: the skip tensor): sc[sample]
// of the workgroup's NS samples for chunk 0, skip[sl] of the samples whose skip tiles this wave holds (downs.1's layout) for chunk 1
template <int NS> struct U1Scales { float sc[NS]; DynScale skip[NS / 2]; };
template <int NS>
__device__ __forceinline__ U1Scales<NS> u1_input_scales(const float* mx, int wave) {
  U1Scales<NS> s;
#pragma unroll
  for (int sm = 0; sm < NS; ++sm) s.sc[sm] = dyn_scale(mx_read(mx, sm)).s;
#pragma unroll
  for (int sl = 0; sl < NS / 2; ++sl) s.skip[sl] = dyn_scale(mx_read(mx, NS / 2 * (wave >> 1) + sl));
  return s;
}
// chunk 0 = ups.0's output (wave w holds channels col = 16 w + n of all NS samples) -> the samples' slabs: block 2 wave + (n >> 3) = (lane
// group wave, chunk n >> 3), the pair (n & ~1, n | 1) one dword; the lanes of a pair swap halves so that each stores whole dwords -- the
// even lane the even positions 2 (4 g + r) of channels (col, col + 1), the odd lane the odd positions of (col - 1, col)
template <int NS>
__device__ __forceinline__ void u1_store_chunk0(char* lb, int wave, int n, int g, const f32x4 (&xe)[NS][1], const f32x4 (&xo)[NS][1],
                                                const float (&sc)[NS]) {
  using GA = U1::GA;
  const bool odd = n & 1;
  char* const d0 = lb + wave * GA::G + (n >> 3) * GA::BX + ((n & 7) >> 1) * 4 + 2 * 16 + (8 * g + (odd ? 1 : 0)) * 16;
#pragma unroll
  for (int sm = 0; sm < NS; ++sm)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float own = (odd ? xo[sm][0][r] : xe[sm][0][r]) * sc[sm];
      const float recv = lane_swap1((odd ? xe[sm][0][r] : xo[sm][0][r]) * sc[sm]);
      const F16Pair p = f16_split2(odd ? recv : own, odd ? own : recv);
      char* d = d0 + sm * U1::W_BYTES + 2 * r * 16;
      *reinterpret_cast<unsigned*>(d) = p.hi;
      MMD_LO(*reinterpret_cast<unsigned*>(d + GA::PS) = p.lo;)
    }
}
// chunk 1 = skip (downs.1's layout: wave = (channel half np, sample pair sp); skip[m][t][r]: sample s0 + (m >> 1), channel 32 np + 2 n + t,
// position 16 (m & 1) + 4 g + r): the lane's channel pair of the 64-channel chunk = block 4 np + (n >> 2) = (chunk (n >> 2) & 1, lane
// group 2 np + (n >> 3)), dword n & 3, in the slabs of the wave's samples
template <int NS>
__device__ __forceinline__ void u1_store_chunk1(char* lb, int wave, int n, int g, const f32x4 (&skip)[NS][2], const DynScale (&sc)[NS / 2]) {
  using GA = U1::GA;
  const int np = wave & 1, s0 = NS / 2 * (wave >> 1);
  char* const sdst = lb + (2 * np + (n >> 3)) * GA::G + ((n >> 2) & 1) * GA::BX + (n & 3) * 4 + (2 + 4 * g) * 16;
#pragma unroll
  for (int m = 0; m < NS; ++m)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const F16Pair p = f16_split2(skip[m][0][r] * sc[m >> 1].s, skip[m][1][r] * sc[m >> 1].s);
      char* d = sdst + (s0 + (m >> 1)) * U1::W_BYTES + (16 * (m & 1) + r) * 16;
      *reinterpret_cast<unsigned*>(d) = p.hi;
      MMD_LO(*reinterpret_cast<unsigned*>(d + GA::PS) = p.lo;)
    }
}
// The transposed tail's output of input tiles m0 .. m0 + MT - 1 (positions 2 m + parity, m = 16 (m0 + mt) + 4 g + r: rows 2 + 32 (m0 + mt)
// + 8 g + 2 r + parity) times s -> the 64-row slab; vsF = slab + the lane's (block n >> 2, row 0, dword n & 3)
template <int MT>
__device__ __forceinline__ void u1_tail_store(char* vsF, int m0, int g, const f32x4 (&e)[MT][2], const f32x4 (&o)[MT][2], float s) {
  using GF [[maybe_unused]] = U1::GF;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const F16Pair pe = f16_split2(e[mt][0][r] * s, e[mt][1][r] * s), po = f16_split2(o[mt][0][r] * s, o[mt][1][r] * s);
      char* d = vsF + (2 + 32 * (m0 + mt) + 8 * g + 2 * r) * 16;
      *reinterpret_cast<unsigned*>(d) = pe.hi;
      MMD_LO(*reinterpret_cast<unsigned*>(d + GF::PS) = pe.lo;)
      *reinterpret_cast<unsigned*>(d + 16) = po.hi;
      MMD_LO(*reinterpret_cast<unsigned*>(d + 16 + GF::PS) = po.lo;)
    }
}
// eps = the 1x1 conv's output times its scale + bias (columns n < 4 of the tile are real), M tiles m0 .. m0 + MT - 1 of a sample:
// ... -> rows [position][4] of et (the sample's slab, for the fused step)
template <int MT>
__device__ __forceinline__ void u1_eps_to_slab(float* et, int m0, int n, int g, const f32x4 (&out)[MT][1], float s1, float b1) {
  if (n < 4) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) et[(16 * (m0 + mt) + 4 * g + r) * 4 + n] = fmaf(out[mt][0][r], s1, b1);
  }
}
// ... -> eps [n, 64, 4] in HBM (the unfused path), sample smp
template <int MT>
__device__ __forceinline__ void u1_store_out(float* eps, size_t smp, int m0, int n, int g, const f32x4 (&out)[MT][1], float s1, float b1) {
  float* dst = eps + (smp * 64 + 16 * m0 + 4 * g) * 4 + n;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int r = 0; r < 4; ++r) dst[(16 * mt + r) * 4] = fmaf(out[mt][0][r], s1, b1);
}
// The unguided ddpm_sample_fn step (sample_functions.py:40-86; ddpm_guide_kernel's arithmetic, guide_dev.h) on trajectory `smp` of the
// launch, in place, lane = support point; et = its eps rows [64][4] in LDS
__device__ __forceinline__ void fused_ddpm_row(const FusedStep& fs, const float* et, int smp, int lane) {
  const float4 e = *reinterpret_cast<const float4*>(et + lane * 4);
  const int traj = fs.traj0 + smp, robot = traj / fs.spr;
  const size_t idx = (size_t)traj * H + lane;
  float4 v = ddpm_posterior_mean(fs.x[idx], e, fs.a_t, fs.b_t, fs.c1, fs.c2);
  if (fs.do_noise)
    v = add_step_noise(v, fs.noise ? fs.noise[idx] : traj_normal4(fs.seed, fs.robot_seeds, fs.draw, fs.traj_base, idx, robot, fs.spr), fs.sigma,
                       fs.noise_std_extra);
  float4 hv;
  if (hard_row(fs.hard_rows, fs.n_hard, fs.hard, robot, lane, hv)) v = hv;
  fs.x[idx] = v;
  if (fs.chain) fs.chain[idx] = v;
}

template <int NS>
__device__ __forceinline__ void chain_body_u1w(const ChainArgs& a, const FinalArgs& f, const FusedStep& fs, float* lds, int n0, int lane_in, int wave,
                                               const f32x4 (&xe)[NS][1], const f32x4 (&xo)[NS][1], const f32x4 (&skip)[NS][2],
                                               int trb, int tb_off = 0) {
  // (an opaque copy of the lane index: the stage's lane-derived offsets are recomputed here -- a handful of VALU ops -- instead
  // of being kept alive, i.e. spilled, since the stages that happen to use the same products)
  int lane = lane_in;
  asm volatile("" : "+v"(lane));
  using GA = U1::GA;
  using GB = U1::GB;
  using GF = U1::GF;
  constexpr int RDA = U1::RDA;
  char* const lb = reinterpret_cast<char*>(lds);
  char* const slab = lb + wave * U1::W_BYTES;
  float* const mx = lds + MX_OFF;
  const int n = lane & 15, g = lane >> 4, c0 = 2 * n;
  auto wt2 = [&](const uint4* w, int frags) { return w_tiles<2>(w, frags, 0, lane); };
  const WTiles<2> wp0 = wt2(a.r0.wa_bf, GA::FRAGS5), wp1 = wt2(a.wa0_c1_bf, GA::FRAGS5);
  const WTiles<2> wr0 = wt2(a.wres_bf, 2 * GA::KC), wr1 = wt2(a.wres_c1_bf, 2 * GA::KC);
  u32x4 ring[RDA][2][2];
  rd_ring_load<GA, 2, RDA>(ring, wp0);
  // ---- the skip tensor's per-sample maxima -> slots 4 .. 7 of mx region 0 (the two waves of a sample pair fill them); ups.0 left its
  //      output's maxima in slots 0 .. 3
  pair_maxima_out<2, 4>(skip, mx, wave, lane);
  __syncthreads();                                           // ups.0 is done with its slabs; the maxima are in mx
  TR(trb + 0);
  const U1Scales<NS> sc = u1_input_scales<NS>(mx, wave);
  const float inv_in = dyn_scale(mx_read(mx, wave)).inv;
  rw_zero_halo<GA>(slab, 32, lane, true);                    // (rows 0, 1, 34, 35 of the own slab's 8 blocks x 2 pieces)
  u1_store_chunk0(lb, wave, n, g, xe, xo, sc.sc);
  TR(trb + 6);
  __syncthreads();
  TR(trb + 7);
  const char* const vaA = slab + g * GA::G + n * 16;
  f32x4 acc[2][2], res[2][2];
  rd_taps<GA, 2, 0, 5, true, true, 2, RDA>(acc, res, vaA, wp0, wr0, ring);
  rd_ring_load<GA, 2, RDA>(ring, wp1);
  TR(trb + 8);
  __syncthreads();                                           // every wave has consumed chunk 0
  u1_store_chunk1(lb, wave, n, g, skip, sc.skip);
  __syncthreads();
  TR(trb + 10);
  float br[2], isr[2];
  const Epi<2> e0a = epi_a_res<2>(a.r0, tb_off, c0, br, isr);
  rd_taps<GA, 2, 0, 5, false, true, 2, RDA>(acc, res, vaA, wp1, wr1, ring);
  TR(trb + 11);
  // ---- from here on the wave is on its own: 32-channel slab
  const char* const vaB = slab + g * GB::G + n * 16;
  char* const vsB = slab + (n >> 2) * GB::G + (2 + 4 * g) * 16 + (n & 3) * 4;
  u32x4 ring5[5][2][2];
  auto preload = [&](const uint4* w) { rd_ring_load<GB, 2, 5>(ring5, wt2(w, GB::FRAGS5)); };
  preload(a.r0.wb_bf);
  auto conv = [&](const uint4* w) {                          // one 32 -> 32 conv over the tile in acc (already scaled)
    const WTiles<2> wp = wt2(w, GB::FRAGS5);
    rw_store2<GB, 2>(vsB, acc);
    wave_lds_fence();
    rd_taps<GB, 2, 0, 5, true, false, 2, 5>(acc, res, vaB, wp, wp, ring5);
    wave_lds_fence();                                        // (the next store must not overtake these reads)
  };
  tile_finish_res(res, isr, inv_in, br);
  rw_gn<2, 128>(acc, e0a, inv_in, a.r0.act_a);
  TR(trb + 1);
  wave_lds_fence();                                          // conv A's reads are done: the slab changes its geometry
  rw_zero_halo<GB>(slab, 32, lane, true);
  {
    const Epi<2> e = epi_b<2>(a.r0, c0);
    conv(a.r0.wb_bf);
    preload(a.ri[0].wa_bf);
    rw_gn<2, 128>(acc, e, 1.f, res);
  }
  TR(trb + 2);
  // ---- identity RTB
  {
    const RtbPtrs& R = a.ri[0];
    tile_copy(res, acc);
    const DynScale ds = dyn_scale(rw_absmax(acc));
    tile_scale(acc, ds.s);
    const Epi<2> ea = epi_a<2>(R, tb_off, c0);
    conv(R.wa_bf);
    preload(R.wb_bf);
    rw_gn<2, 128>(acc, ea, ds.inv, R.act_a);
    TR(trb + 3);
    const Epi<2> eb = epi_b<2>(R, c0);
    conv(R.wb_bf);
    rw_gn<2, 128>(acc, eb, 1.f, res);
    TR(trb + 4);
  }
  // ---- tail: Upsample1d = ConvTranspose1d(k4, s2, p1): out[2 m] = in[m - 1] W3 + in[m] W1, out[2 m + 1] = in[m] W2 + in[m + 1] W0
  //      -> the final block's input (L = 64) in the 64-row slab
  const char* const vaF = slab + g * GF::G + n * 16;
  char* const vsF = slab + (n >> 2) * GF::G + (n & 3) * 4;
  f32x4 y[4][2];
  float inv_f;
  {
    const DynScale ds = dyn_scale(rw_absmax(acc));
    tile_scale(acc, ds.s);
    const WTiles<2> wt0 = wt2(a.wt_bf0, 2 * GB::KC * 2), wt1 = wt2(a.wt_bf1, 2 * GB::KC * 2);
    u32x4 ring2[2][2][2];
    const TailRec<2, 2> tl = tail_rec<2, 2>(a.rt, c0);
    const float is0[2] = {tl.is[0][0] * ds.inv, tl.is[0][1] * ds.inv}, is1[2] = {tl.is[1][0] * ds.inv, tl.is[1][1] * ds.inv};
    rd_ring_load<GB, 2, 2>(ring2, wt0);
    rw_store2<GB, 2>(vsB, acc);
    wave_lds_fence();
    f32x4 e[2][2], o[2][2];
    rd_taps<GB, 2, 1, 2, true, false, 2, 2>(e, res, vaB, wt0, wt0, ring2);
    rd_ring_load<GB, 2, 2>(ring2, wt1);
    rd_taps<GB, 2, 2, 2, true, false, 2, 2>(o, res, vaB, wt1, wt1, ring2);
    const DynScale df = dyn_scale(tail_up_epilogue(e, o, is0, is1, tl.bt));
    inv_f = df.inv;
    wave_lds_fence();                                        // the tail's reads are done: 64-row geometry
    rw_zero_halo<GF>(slab, 64, lane, true);
    u1_tail_store<2>(vsF, 0, g, e, o, df.s);
  }
  TR(trb + 5);
  // ---- final block: Conv1dBlock(32 -> 32, k5) + GroupNorm + Mish, then the 1x1 conv 32 -> 4 (N padded to one n-tile)
  {
    const WTiles<2> wf = wt2(f.w5, GF::FRAGS5);
    rd_ring_load<GF, 2, 5>(ring5, wf);
    const WTiles<1> w1 = w_tiles<1>(f.w1_bf, 2 * GF::KC, 0, lane);
    u32x4 ring1[1][1][2];
    rd_ring_load<GF, 1, 1>(ring1, w1);
    const Epi<2> ef = epi_rec<2>(f.rec5, nullptr, c0);
    const float2 o1 = *reinterpret_cast<const float2*>(f.rec1 + (n & 3) * 4);
    const float b1 = o1.x, s1 = o1.y;
    wave_lds_fence();
    rd_taps<GF, 2, 0, 5, true, false, 4, 5>(y, y, vaF, wf, wf, ring5);
    rw_gn_mish_whole<4, 2, 2, 256, true>(y, ef.b, ef.g, ef.be, ef.is, inv_f, act_scale(f.act), [](int, int, int) { return 0.f; });
    wave_lds_fence();
    rw_store2<GF, 4>(vsF + (2 + 4 * g) * 16, y);
    wave_lds_fence();
    f32x4 out[4][1];
    rd_taps<GF, 1, 2, 1, true, false, 4, 1>(out, out, vaF, w1, w1, ring1);
    auto valid = [&] { return wave < NS && n0 + wave < a.n; };   // (a.n is read inside the branch that needs it)
    if (fs.enabled) {
      // eps[64][4] -> the wave's slab as float4 rows, then the fused step on the wave's trajectory
      float* const et = reinterpret_cast<float*>(slab);
      wave_lds_fence();                                      // (the 1x1 conv's reads of the slab are done)
      u1_eps_to_slab<4>(et, 0, n, g, out, s1, b1);
      wave_lds_fence();
      if (valid()) fused_ddpm_row(fs, et, n0 + wave, lane);
    } else if (n < 4 && valid()) {
      u1_store_out<4>(f.out, n0 + wave, 0, n, g, out, s1, b1);
    }
  }
}

// ups.1 + final block for unet_kernel<2>: like chain_body_d0s a sample is split between two waves by position (wave = (sample sp =
// wave >> 1, half hf = wave & 1): ONE M tile of the L = 32 convs, two of the final block's L = 64), the sample's slab is shared,
// GroupNorm statistics / dynamic scales are exchanged through LDS, weights are staged through LDS one conv ahead (stage_weights: two
// buffers behind the two samples' slabs).  The two input chunks arrive across waves as in chain_body_u1w (downs.1's skip layout for
// two trajectories has the same sample index sp, and np = hf).
template <int NV>
__device__ __forceinline__ void chain_body_u1s(const ChainArgs& a, const FinalArgs& f, const FusedStep& fs, float* lds, int n0, int lane_in, int wave,
                                               const f32x4 (&xe)[2][1], const f32x4 (&xo)[2][1], const f32x4 (&skip)[2][2], int trb, int tb_off = 0) {
  int lane = lane_in;
  asm volatile("" : "+v"(lane));
  using GA = U1::GA;
  using GB = U1::GB;
  using GF = U1::GF;
  constexpr int RDA = U1::RDA, TF = U1::TF;
  char* const lb = reinterpret_cast<char*>(lds);
  const int sp = wave >> 1, hf = wave & 1;
  char* const slab = lb + sp * U1::W_BYTES;
  float* const mx = lds + MX_OFF;
  const RwHalf half{reinterpret_cast<HalfStat*>(lds + PARK2_OFF) + sp * 128, hf, lane};
  const int n = lane & 15, g = lane >> 4, c0 = 2 * n;
  auto wt2 = [&](const uint4* w, int frags) { return w_tiles<2>(w, frags, 0, lane); };
  const WTiles<2> wp0 = wt2(a.r0.wa_bf, GA::FRAGS5), wp1 = wt2(a.wa0_c1_bf, GA::FRAGS5);
  const WTiles<2> wr0 = wt2(a.wres_bf, 2 * GA::KC), wr1 = wt2(a.wres_c1_bf, 2 * GA::KC);
  u32x4 ring[RDA][2][2];
  rd_ring_load<GA, 2, RDA>(ring, wp0);
  // ---- the skip tensor's per-sample maxima -> slots 4 .. 7 of mx region 0; ups.0 left its output's maxima in slots 0 .. 3
  pair_maxima_out<2, 4>(skip, mx, wave, lane);
  __syncthreads();                                           // ups.0 is done with its slabs; the maxima are in mx
  TR(trb + 0);
  char* const wb0 = lb + 2 * U1::W_BYTES;
  char* const wb1 = wb0 + WBUF_BYTES;
  stage_weights<2 * GB::FRAGS5>(a.r0.wb_bf, wb0, wave, lane);     // RTB 0's conv B lands while conv A runs
  const U1Scales<2> sc = u1_input_scales<2>(mx, wave);
  const float inv_in = sc.skip[0].inv;                       // (the wave's sample is the one whose skip tiles it holds)
  rw_zero_halo<GA>(slab, 32, lane, hf == 0);                 // (the sample's slab, 8 blocks x 2 pieces: one wave per sample)
  u1_store_chunk0(lb, wave, n, g, xe, xo, sc.sc);
  TR(trb + 6);
  __syncthreads();
  TR(trb + 7);
  const char* const vaA = slab + g * GA::G + (n + 16 * hf) * 16;
  f32x4 acc[1][2], res[1][2];
  rd_taps<GA, 2, 0, 5, true, true, 1, RDA>(acc, res, vaA, wp0, wr0, ring);
  rd_ring_load<GA, 2, RDA>(ring, wp1);
  TR(trb + 8);
  __syncthreads();                                           // every wave has consumed chunk 0
  u1_store_chunk1(lb, wave, n, g, skip, sc.skip);
  __syncthreads();
  TR(trb + 10);
  float br[2], isr[2];
  const Epi<2> e0a = epi_a_res<2>(a.r0, tb_off, c0, br, isr);
  rd_taps<GA, 2, 0, 5, false, true, 1, RDA>(acc, res, vaA, wp1, wr1, ring);
  TR(trb + 11);
  // ---- 32-channel slab of the sample, shared by its two waves
  const char* const vaB = slab + g * GB::G + (n + 16 * hf) * 16;
  char* const vsB = slab + (n >> 2) * GB::G + (2 + 4 * g + 16 * hf) * 16 + (n & 3) * 4;
  u32x4 ring2[2][2][2];
  // one 32 -> 32 conv over the half tile in acc (already scaled), its weights staged in wb; `stage_next` puts the next conv's on
  // their way behind the barrier (every wave is past the conv that read the other buffer)
  auto conv = [&](char* wb, auto stage_next) {
    const WStaged<2> wp = w_staged<2>(wb, GB::FRAGS5, lane);
    rw_store2<GB, 1>(vsB, acc);
    staged_weights_landed();
    __syncthreads();
    stage_next();
    rd_ring_load<GB, 2, 2>(ring2, wp);
    rd_taps<GB, 2, 0, 5, true, false, 1, 2>(acc, res, vaB, wp, wp, ring2);
  };
  tile_finish_res(res, isr, inv_in, br);
  rw_gn<2, 128>(acc, e0a, inv_in, a.r0.act_a, half);         // (its barrier: conv A's reads are done, the slab changes its geometry)
  TR(trb + 1);
  rw_zero_halo<GB>(slab, 32, lane, hf == 0);
  {
    const Epi<2> e = epi_b<2>(a.r0, c0);
    conv(wb0, [&] { stage_weights<2 * GB::FRAGS5>(a.ri[0].wa_bf, wb1, wave, lane); });
    rw_gn<2, 128>(acc, e, 1.f, res, half);
  }
  TR(trb + 2);
  // ---- identity RTB
  {
    const RtbPtrs& R = a.ri[0];
    tile_copy(res, acc);
    const DynScale ds = dyn_scale(half_sample_max(mx, sp, hf, lane, rw_absmax(acc)));
    tile_scale(acc, ds.s);
    const Epi<2> ea = epi_a<2>(R, tb_off, c0);
    conv(wb1, [&] { stage_weights<2 * GB::FRAGS5>(R.wb_bf, wb0, wave, lane); });
    rw_gn<2, 128>(acc, ea, ds.inv, R.act_a, half);
    TR(trb + 3);
    const Epi<2> eb = epi_b<2>(R, c0);
    conv(wb0, [&] {                                          // the tail's two parity passes
      stage_weights<TF>(a.wt_bf0, wb1, wave, lane);
      stage_weights<TF>(a.wt_bf1, wb1 + TF * 1024, wave, lane);
    });
    rw_gn<2, 128>(acc, eb, 1.f, res, half);
    TR(trb + 4);
  }
  // ---- tail: Upsample1d as two parity passes -> the final block's input (L = 64), the half's rows of the 64-row slab
  const char* const vaF = slab + g * GF::G + (n + 32 * hf) * 16;
  char* const vsF = slab + (n >> 2) * GF::G + (n & 3) * 4;
  f32x4 y[2][2];
  float inv_f;
  {
    const DynScale ds = dyn_scale(half_sample_max(mx, sp, hf, lane, rw_absmax(acc)));
    tile_scale(acc, ds.s);
    const WStaged<2> wt0 = w_staged<2>(wb1, TF / 2, lane), wt1 = w_staged<2>(wb1 + TF * 1024, TF / 2, lane);
    const TailRec<2, 2> tl = tail_rec<2, 2>(a.rt, c0);
    const float is0[2] = {tl.is[0][0] * ds.inv, tl.is[0][1] * ds.inv}, is1[2] = {tl.is[1][0] * ds.inv, tl.is[1][1] * ds.inv};
    rw_store2<GB, 1>(vsB, acc);
    staged_weights_landed();
    __syncthreads();
    stage_weights<2 * GF::FRAGS5>(f.w5, wb0, wave, lane);    // the final block's k5 conv
    f32x4 e[1][2], o[1][2];
    rd_ring_load<GB, 2, 2>(ring2, wt0);
    rd_taps<GB, 2, 1, 2, true, false, 1, 2>(e, res, vaB, wt0, wt0, ring2);
    rd_ring_load<GB, 2, 2>(ring2, wt1);
    rd_taps<GB, 2, 2, 2, true, false, 1, 2>(o, res, vaB, wt1, wt1, ring2);
    const float m = tail_up_epilogue(e, o, is0, is1, tl.bt);
    const DynScale df = dyn_scale(half_sample_max(mx, sp, hf, lane, m));   // (its barrier: the tail's reads are done, 64-row geometry)
    inv_f = df.inv;
    rw_zero_halo<GF>(slab, 64, lane, hf == 0);
    u1_tail_store<1>(vsF, hf, g, e, o, df.s);
  }
  TR(trb + 5);
  // ---- final block: Conv1dBlock(32 -> 32, k5) + GroupNorm + Mish, then the 1x1 conv 32 -> 4, on the half's two M tiles
  {
    const WStaged<2> wf = w_staged<2>(wb0, GF::FRAGS5, lane);
    const WTiles<1> w1 = w_tiles<1>(f.w1_bf, 2 * GF::KC, 0, lane);
    u32x4 ring1[1][1][2];
    rd_ring_load<GF, 1, 1>(ring1, w1);
    const Epi<2> ef = epi_rec<2>(f.rec5, nullptr, c0);
    const float2 o1 = *reinterpret_cast<const float2*>(f.rec1 + (n & 3) * 4);
    const float b1 = o1.x, s1 = o1.y;
    staged_weights_landed();
    __syncthreads();                                         // the final block's input and weights are complete
    rd_ring_load<GF, 2, 2>(ring2, wf);
    rd_taps<GF, 2, 0, 5, true, false, 2, 2>(y, y, vaF, wf, wf, ring2);
    rw_gn_mish_half<2, 2, 2, 256, true>(y, ef.b, ef.g, ef.be, ef.is, inv_f, act_scale(f.act), [](int, int, int) { return 0.f; }, half.xch, hf, lane);
    // (the exchange's barrier: the partner is past its taps, the slab may be overwritten; the 1x1 conv reads only the centre
    // tap = the wave's own rows)
    rw_store2<GF, 2>(vsF + (2 + 4 * g + 32 * hf) * 16, y);
    wave_lds_fence();
    f32x4 out[2][1];
    rd_taps<GF, 1, 2, 1, true, false, 2, 1>(out, out, vaF, w1, w1, ring1);
    auto valid = [&] { return sp < NV && n0 + sp < a.n; };
    if (fs.enabled) {
      // eps[64][4] -> the sample's slab as float4 rows (both waves their halves), then the fused step on the trajectory by the sample's
      // first wave
      float* const et = reinterpret_cast<float*>(slab);
      __syncthreads();                                       // (both waves' 1x1 reads of the slab are done)
      u1_eps_to_slab<2>(et, 2 * hf, n, g, out, s1, b1);
      __syncthreads();
      if (hf == 0 && valid()) fused_ddpm_row(fs, et, n0 + sp, lane);
    } else if (n < 4 && valid()) {
      u1_store_out<2>(f.out, n0 + sp, 2 * hf, n, g, out, s1, b1);
    }
  }
}

// ----------------------------------------------------------------------------------------------------------------
// The whole TemporalUnet forward for 4 samples in ONE workgroup / ONE launch: the five level chains and the final conv
// hand their activations to each other through LDS (tail tile -> next stage's x slab), the two skip connections wait in
// registers (32 VGPRs each) for the up path.  HBM traffic per trajectory and forward: 1 KiB in, 1 KiB out.
// ----------------------------------------------------------------------------------------------------------------
struct UnetArgs {
  ChainArgs c[5];
  FinalArgs fin;
  int n;
  FusedStep fs;           // enabled: the unguided DDPM step on the launch's trajectories follows in the same kernel
};

// NS = trajectories per workgroup.  4: the form everything above is written for.  2 (launched for small batches, which leave
// most CUs without a workgroup otherwise: twice the workgroups): only samples 0, 1 exist -- the L = 16 stages (downs.2 + mid,
// ups.0: 3/4 of the matrix work, waves = channel slices x ALL samples) run over two samples, i.e. half the MFMAs, A reads,
// epilogue and parking per wave for the same weight stream, downs.1's waves (n-tile pair x sample PAIR) take one sample each,
// and the stages whose waves ARE samples at NS = 4 (downs.0, ups.1 + final block) split a sample between two waves (chain_body_d0s /
// u1s).  Per-sample arithmetic is the same instruction sequence either way: the results are bitwise equal.
// tb_off: added to every RTB's time-bias pointer (floats) -- 0 in unet_kernel, whose host side bakes the step's row of the time
// table into the pointers; t * tb_total in the persistent kernel, whose pointers are those of row 0
// 1 (unet_kernel<1>, launches of <= ns1_max = 256 trajectories -- one workgroup per CU at most; ONE planner call has 64): the L = 16 stages
// run ONE M tile per conv -- the conv's time there is the weight
// stream plus what the samples' MFMAs, A-fragment reads and epilogues add to it: 3.15 -> 2.7 us per 128 -> 128 conv at <= 64 workgroups
// (tools/ubench/pair_split.hip, arms basePF / base1PF) -- while the stages whose waves are sample halves or n-tile pairs x samples
// (downs.0, downs.1, ups.1 + final block) keep the two-trajectory form (NP = 2 below) with sample 1 fed zeros and never stored.  A
// sample's arithmetic is the same instruction sequence: bitwise the results of unet_kernel<2> / <4>.
template <int NS>
__device__ __forceinline__ void unet_forward_body(const UnetArgs& a, const FusedStep& fs, int tb_off, float* lds, int n0, int lane, int wave) {
  constexpr int NP = NS == 1 ? 2 : NS;                       // samples of downs.0, downs.1 and ups.1 + final block
  f32x4 skip1[NP][2], skip2[NS][2], xe[NP][1], xo[NP][1];
  if constexpr (NS == 1) {
#pragma unroll
    for (int r = 0; r < 4; ++r) xe[1][0][r] = xo[1][0][r] = 0.f;
  }
  // ---- downs.0 @ L=64 -> [4][32][32]: direct f16x2 convs on per-sample slabs, wave = sample or half a sample
  if constexpr (NS <= 2) chain_body_d0s<NS>(a.c[0], lds, n0, lane, wave, 0, tb_off);
  else chain_body_d0w<NS>(a.c[0], lds, n0, lane, wave, 0, tb_off);
  // ---- downs.1 @ L=32 -> [4][16][64], skip1: direct f16x2 convs, wave = (n-tile pair, sample pair) (chain_body_d1d)
  chain_body_d1d<NP>(a.c[1], lds, lane, wave, skip1, 40, tb_off);
  // ---- downs.2 + mid blocks @ L=16 -> [NS][16][128], skip2: direct f16x2 convs (chain_body_d2d; lane = channels 32 wave + 2
  //      (lane & 15) + h, positions 4 (lane >> 4) + r of all NS samples)
  f32x4 mid_out[NS][2];
  chain_body_d2d<NS>(a.c[2], lds, lane, wave, mid_out, skip2, 80, tb_off);
  TR(130);
  // ---- ups.0 @ L=16: cat(x, skip2) -> [NS][32][64] (chain_body_u0d; the chunks are stored from downs.2's tiles); its output
  //      stays in registers (even / odd positions of channel 16 wave + (lane & 15))
  {
    using G128 = RdGeo<128>;
    char* const slab128 = reinterpret_cast<char*>(lds) + D2::SLAB_OFF;
    char* const vs = slab128 + wave * G128::G + ((lane & 15) >> 2) * G128::BX + (2 + 4 * (lane >> 4)) * 16 + (lane & 3) * 4;
    chain_body_u0d<NS>(a.c[3], lds, lane, wave, mid_out, skip2, [&](const f32x4 (&t)[NS][2]) { rd_store2<G128>(vs, t); }, slab128,
                       sub_tile<NS>(xe, 0), sub_tile<NS>(xo, 0), 136, tb_off);
  }
  TR(131);
  // ---- ups.1 @ L=32: cat(x, skip1) -> [4][64][32], final_conv: Conv1dBlock(32->32) -> 1x1 conv (32->4) -> eps[n,64,4]
  if constexpr (NS <= 2) chain_body_u1s<NS>(a.c[4], a.fin, fs, lds, n0, lane, wave, xe, xo, skip1, 146, tb_off);
  else chain_body_u1w<NS>(a.c[4], a.fin, fs, lds, n0, lane, wave, xe, xo, skip1, 146, tb_off);
  TR(133);
}

template <int NS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void unet_kernel(UnetArgs a) {
  __shared__ __attribute__((aligned(16))) float lds[UNET_LDS_FLOATS];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  unet_forward_body<NS>(a, a.fs, 0, lds, blockIdx.x * NS, lane, wave);
}

// A RUN of consecutive unguided DDPM steps in ONE launch (mmd_p_sample_loop: the steps before guidance starts, or every step of a
// prior-only call): a workgroup iterates the steps of its own NS trajectories -- forward, fused ddpm_sample_fn step (the wave that
// holds a trajectory's eps writes x in place), the next forward reads what the same workgroup wrote.  No launch boundary between
// the steps: no dispatch gap, and the workgroups of a CU never wait for the slowest workgroup of the chip.  sc[s]: the step's
// schedule coefficients and its row of the time table (a.c[*].*.tb point at row 0); chain / injected noise advance by one
// batch per step.  Same arithmetic as the launch-per-step form: bitwise-equal results.
// The argument block comes through a pointer into the constant address space, re-derived from an opaque integer every step: as
// by-value kernel arguments inside a loop the ~300 pointers were hoisted out of it, i.e. kept -- spilled -- across the whole forward
// (1100 VGPR spills); loaded where they are used (s_load from a uniform address) the loop body compiles like unet_kernel's.
static_assert(sizeof(UnetArgs) <= PERSIST_TABLE_BYTES - PERSIST_ARGS_OFF, "the argument block fits its workspace region");
template <int NS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void unet_persist_kernel(const UnetArgs* ap, const FusedStep* steps,
                                                                                                     int n_steps, int tb_total) {
  __shared__ __attribute__((aligned(16))) float lds[UNET_LDS_FLOATS];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  typedef const __attribute__((address_space(4))) UnetArgs* ConstArgs;
  typedef const __attribute__((address_space(4))) FusedStep* ConstStep;
  for (int s = 0; s < n_steps; ++s) {
    unsigned long long pa = reinterpret_cast<unsigned long long>(ap), ps = reinterpret_cast<unsigned long long>(steps + s);
    asm volatile("" : "+s"(pa), "+s"(ps));
    const UnetArgs& a = *(const UnetArgs*)(ConstArgs)pa;
    const FusedStep& fs = *(const FusedStep*)(ConstStep)ps;     // (read where the fused step uses it: the tail of the forward)
    // (an opaque copy of the lane index per step: lane-derived slab offsets are loop invariant, and hoisted out of the loop they
    // would stay live -- spilled -- across the whole forward)
    int lane_s = lane;
    asm volatile("" : "+v"(lane_s));
    unet_forward_body<NS>(a, fs, fs.t_row * tb_total, lds, blockIdx.x * NS, lane_s, wave);
    // every wave is done with the LDS of this step, and the trajectories the workgroup wrote are visible to all of its waves
    // (unet_kernel<2>: a sample's second wave reads what its first wave stored)
    __threadfence_block();
    __syncthreads();
  }
}

#ifdef MMD_UNET_F16
}  // namespace f16
#endif
}  // namespace mmd
