// The vector-ALU kernels of the layer-by-layer TemporalUnet (host side: unet_layers.hip): plain fp32 FMA arithmetic, activations
// channels-FIRST [n][C][L] (the trajectory input and the eps output channels-last [n][L][4]).  They run every layer of a network whose
// widths have no whole 16-column n-tiles or GroupNorm groups (unet_input_dim 8 / 24 / 40 / 56, MMD_UNET_LAYERED_VALU), and the final
// 1x1 conv to eps of every network.
//
// conv5_block_kernel (a Conv1dBlock): a workgroup owns one sample and a slice of whole GroupNorm groups of the output channels
// (blockIdx.y; small launches are split 2 .. 8 ways so they still fill the chip).  The input rows are staged in LDS as [c_in][L + 8] with
// four zeros either side (no boundary tests in the loop); a thread holds a register tile of 4 positions x CT channels: per input channel
// it reads its 8-position window once (two 16-byte LDS reads) and 5 CT weights [tap][c_in][c_out] (adjacent threads = adjacent output
// channels: coalesced, L2-resident) for 20 CT FMAs.  The conv output goes to LDS for the GroupNorm (8 groups, two-pass statistics, eps
// 1e-5) + Mish + addend, then to HBM.
// conv_plain_kernel: the strided / transposed / 1x1 convs without a norm, one thread per output, split over blockIdx.y likewise.
#pragma once
#include <hip/hip_runtime.h>

namespace mmd {

namespace {

constexpr int N_GROUPS = 8;                    // group_norm_n_groups(c) = 8 for every multiple of 8 (layers.py:392-398)

__device__ __forceinline__ float mish_ref(float y) {          // torch.nn.Mish: y tanh(softplus(y)), softplus threshold 20
  const float sp = y > 20.f ? y : log1pf(expf(y));
  return y * tanhf(sp);
}

struct ConvArgs {
  const float* x1; const float* x2;   // input [n][C1][L_in] (+ [n][C2][L_in] concatenated behind it along the channels, or NULL)
  int c1, c2, l_in, l_out, c_out;
  int cs;                             // output channels per workgroup (blockIdx.y * cs = first)
  int in_cl, out_cl;                  // the input / output tensor is channels-last [n][L][C] (the trajectory, eps)
  const float* wt;                    // [taps][c1 + c2][c_out]
  const float* bias;                  // [c_out]
  const float* gamma; const float* beta;   // GroupNorm affine (conv5_block_kernel)
  const float* add_c;                 // per-channel addend after Mish (time bias), or NULL
  const float* add_t;                 // [n][c_out][l_out] addend after Mish (residual), or NULL
  float* y;                           // [n][c_out][l_out]
  int in_bl;                          // x1 is a blocked activation tensor [n][c1 / 8][l_in][8] of the matrix-pipe path (mconv_kernel)
};

// element offset of (sample, channel c, position l) in a blocked activation tensor of C channels
__device__ __forceinline__ size_t bl_off(size_t smp, int C, int L, int c, int l) { return ((smp * (C >> 3) + (c >> 3)) * L + l) * 8 + (c & 7); }
__device__ __forceinline__ float load_in(const ConvArgs& a, size_t n, int c, int l) {
  if (a.in_bl) return a.x1[bl_off(n, a.c1, a.l_in, c, l)];
  if (a.in_cl) return a.x1[(n * a.l_in + l) * a.c1 + c];
  return c < a.c1 ? a.x1[(n * a.c1 + c) * a.l_in + l] : a.x2[(n * a.c2 + (c - a.c1)) * a.l_in + l];
}

// Conv1dBlock (layers.py:232-258): Conv1d(k5, p2) -> GroupNorm(8) -> Mish, + per-channel addend, + tensor addend.
// blockDim = KS * NT, NT = min(64, the slice's (L / 4) * (cs / CT) register tiles rounded up to 16): always whole waves, at most
// 256 threads; a thread loops over the tiles r, r + NT, ... of its thread group (one trip for the power-of-two channel counts, more
// where a GroupNorm group is 5 or 7 channels wide: unet_input_dim 40 / 56).  The sum over the input channels is DEFINED as KS = 4
// interleaved partial sums (channels ci = r mod 4, taps in order) combined as ((s0 + s1) + (s2 + s3)) + bias: thread group r of a
// workgroup computes s_r, so the bits do not depend on how a launch is sliced (CT, cs follow the batch size).
constexpr int KS = 4;
template <int CT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 4))) void conv5_block_kernel(ConvArgs a) {
  extern __shared__ float lds[];
  const int cin = a.c1 + a.c2, L = a.l_in, Lp = L + 8, tid = threadIdx.x, nthr = blockDim.x;
  const size_t n = blockIdx.x;
  const int c0 = blockIdx.y * a.cs, tile = a.cs * L;
  float* xs = lds;                               // [cin][Lp]
  float* part = lds + cin * Lp;                  // [KS][cs][L] partial sums; [0] becomes the conv output
  float* red = part + KS * tile;                 // [2 * groups of the slice]
  for (int i = tid; i < cin * Lp; i += nthr) {
    const int c = i / Lp, l = i % Lp - 4;
    xs[i] = (l >= 0 && l < L) ? load_in(a, n, c, l) : 0.f;
  }
  __syncthreads();
  const int lanes = a.cs / CT, items = (L / 4) * lanes, nt = nthr / KS, ks = tid / nt;
  for (int r = tid % nt; r < items; r += nt) {
    const int cl = r % lanes, pg = r / lanes;
    float acc[CT][4];
#pragma unroll
    for (int j = 0; j < CT; ++j)
#pragma unroll
      for (int p = 0; p < 4; ++p) acc[j][p] = 0.f;
    // weight loads through a buffer descriptor: a per-thread byte offset (input channel ks, output channel lane cl) that never
    // changes + a scalar offset per (iteration, tap, channel tile): no vector address arithmetic in the loop
    const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.wt), 0, 5 * cin * a.c_out * 4, 0x00020000);
    const int voff = 4 * (ks * a.c_out + cl * CT);                 // the thread's CT output channels are adjacent: one load per tap
    const int tap = cin * a.c_out;
    auto load_w = [&](float (&w)[5 * CT], int it) {
      const int so = c0 + it * KS * a.c_out;
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        if constexpr (CT == 1) {
          w[k] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(wrs, voff, 4 * (so + k * tap), 0));
        } else if constexpr (CT == 2) {
          // (the b64 / b128 buffer-load builtins of this compiler return the first dword in every component: plain vector loads)
          const float2 v = *reinterpret_cast<const float2*>(reinterpret_cast<const char*>(a.wt + so + k * tap) + voff);
          w[2 * k] = v.x; w[2 * k + 1] = v.y;
        } else {
          const float4 v = *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(a.wt + so + k * tap) + voff);
          w[4 * k] = v.x; w[4 * k + 1] = v.y; w[4 * k + 2] = v.z; w[4 * k + 3] = v.w;
        }
      }
    };
    auto taps = [&](const float (&w)[5 * CT], int ci) {
      const float4* xr = reinterpret_cast<const float4*>(xs + ci * Lp + pg * 4);     // positions 4 pg - 4 .. 4 pg + 7
      const float4 v0 = xr[0], v1 = xr[1], v2 = xr[2];
      const float xw[8] = {v0.z, v0.w, v1.x, v1.y, v1.z, v1.w, v2.x, v2.y};           // positions 4 pg - 2 .. 4 pg + 5
#pragma unroll
      for (int k = 0; k < 5; ++k)
#pragma unroll
        for (int j = 0; j < CT; ++j)
#pragma unroll
          for (int p = 0; p < 4; ++p) acc[j][p] = fmaf(xw[p + k], w[k * CT + j], acc[j][p]);
    };
    // two weight sets in flight alternately: the next input channel's loads are issued before the current one's 20 CT FMAs
    float w0[5 * CT], w1[5 * CT];
    const int nci = cin / KS;                            // this thread's input channels: ks, ks + KS, ... (c_in is 4 or a multiple of 8)
    if (nci > 0) load_w(w0, 0);
    int it = 0;
    for (; it + 2 <= nci; it += 2) {
      load_w(w1, it + 1);
      taps(w0, ks + it * KS);
      load_w(w0, it + 2 < nci ? it + 2 : it);
      taps(w1, ks + (it + 1) * KS);
    }
    if (it < nci) taps(w0, ks + it * KS);
#pragma unroll
    for (int j = 0; j < CT; ++j)
      *reinterpret_cast<float4*>(part + ks * tile + (cl * CT + j) * L + pg * 4) =
          make_float4(acc[j][0], acc[j][1], acc[j][2], acc[j][3]);
  }
  __syncthreads();
  float* outs = part;
  for (int o = tid; o < tile; o += nthr)                // (each element is read and written by the same thread)
    outs[o] = ((part[o] + part[tile + o]) + (part[2 * tile + o] + part[3 * tile + o])) + a.bias[c0 + o / L];
  __syncthreads();
  // GroupNorm over (c_out / 8 channels) x L positions per group = one contiguous block of `outs`; a wave per group
  const int cpg = a.c_out / N_GROUPS, per = cpg * L, lane = tid & 63, wave = tid >> 6, nwave = nthr >> 6;
  for (int g = wave; g < a.cs / cpg; g += nwave) {
    const float* blk = outs + g * per;
    float s = 0.f;
    for (int i = lane; i < per; i += 64) s += blk[i];
    for (int off = 32; off; off >>= 1) s += __shfl_xor(s, off);
    const float mean = s / (float)per;
    float q = 0.f;
    for (int i = lane; i < per; i += 64) {
      const float d = blk[i] - mean;
      q = fmaf(d, d, q);
    }
    for (int off = 32; off; off >>= 1) q += __shfl_xor(q, off);
    if (lane == 0) {
      red[2 * g] = mean;
      red[2 * g + 1] = 1.f / sqrtf(q / (float)per + 1e-5f);
    }
  }
  __syncthreads();
  const size_t base = (n * a.c_out + c0) * L;
  for (int o = tid; o < tile; o += nthr) {
    const int c = o / L, co = c0 + c, g = c / cpg;
    float v = mish_ref((outs[o] - red[2 * g]) * red[2 * g + 1] * a.gamma[co] + a.beta[co]);
    if (a.add_c) v += a.add_c[co];
    if (a.add_t) v += a.add_t[base + o];
    a.y[base + o] = v;
  }
}

// MODE 0: Conv1d, K taps, stride S, padding K / 2.  MODE 1: ConvTranspose1d(k4, s2, p1): out[2 m] = in[m - 1] W3 + in[m] W1,
// out[2 m + 1] = in[m] W2 + in[m + 1] W0 (taps stored in kernel-index order 0 .. 3).  No norm; input staged as [l][c_in].
template <int MODE, int K, int S>
__global__ __launch_bounds__(256) void conv_plain_kernel(ConvArgs a) {
  extern __shared__ float lds[];
  const int cin = a.c1 + a.c2, tid = threadIdx.x;
  const size_t n = blockIdx.x;
  const int c0 = blockIdx.y * a.cs;
  float* xin = lds;                              // [l_in][cin]
  for (int i = tid; i < a.l_in * cin; i += 256) {
    const int c = a.in_cl ? i % cin : i / a.l_in, l = a.in_cl ? i / cin : i % a.l_in;
    xin[l * cin + c] = load_in(a, n, c, l);
  }
  __syncthreads();
  for (int o = tid; o < a.l_out * a.cs; o += 256) {
    // adjacent threads = adjacent output channels (coalesced weights); the store below is strided but small
    const int lo = o / a.cs, co = c0 + o % a.cs;
    float acc = a.bias[co];
    if (MODE == 0) {
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const int li = lo * S + k - K / 2;
        if (li < 0 || li >= a.l_in) continue;
        const float* xr = xin + li * cin;
        const float* wr = a.wt + (size_t)k * cin * a.c_out + co;
        for (int ci = 0; ci < cin; ++ci) acc = fmaf(xr[ci], wr[(size_t)ci * a.c_out], acc);
      }
    } else {
      const int m = lo >> 1, par = lo & 1;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int li = par ? m + j : m - 1 + j;            // parity 0: (m - 1, W3), (m, W1); parity 1: (m, W2), (m + 1, W0)
        const int k = par ? 2 - 2 * j : 3 - 2 * j;
        if (li < 0 || li >= a.l_in) continue;
        const float* xr = xin + li * cin;
        const float* wr = a.wt + (size_t)k * cin * a.c_out + co;
        for (int ci = 0; ci < cin; ++ci) acc = fmaf(xr[ci], wr[(size_t)ci * a.c_out], acc);
      }
    }
    if (a.out_cl) a.y[(n * a.l_out + lo) * a.c_out + co] = acc;
    else a.y[(n * a.c_out + co) * a.l_out + lo] = acc;
  }
}

}  // namespace

}  // namespace mmd
