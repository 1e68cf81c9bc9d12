// Quantized update exchange (QSGD: Alistarh et al., NeurIPS 2017; error feedback: Karimireddy et
// al., ICML 2019): a client's round update w - anchor (+ its residual) leaves as int8 or int4 codes
// with one fp32 scale per group of 64 elements, and the mean of M such payloads is decoded onto the
// anchor, in bandwidth-bound passes over the fp32 arena (gfx950).  parallel/compress.py holds the
// specification (torch_quantize_, torch_decode_mean_); the kernels equal it bit for bit.
//
//   fd_quant_encode       one streaming pass.  A lane takes 32 bits of codes: 4 elements (one float4)
//                         at int8, 8 elements (two float4) at int4, so a group of 64 elements is 16
//                         resp. 8 consecutive lanes.  v = (w - anchor) + e; the group's max |v| is the
//                         unsigned max of the |v| bit patterns (exact; an inf or NaN sorts above every
//                         finite value) through xor-shuffles over 1/2/4(/8), which stay inside the
//                         aligned lane group; n % 64 == 0 makes a group's lanes enter and leave the
//                         grid-stride loop together, so no lane reads an inactive one.
//                           a == 0, a not finite, or inv = qmax / a not finite: the group is empty --
//                           scale +0, codes 0, e' = v (a not finite: the group is bad, e' = +0);
//                           otherwise s = a / qmax, t = v * inv, q = clamp(floor(t + u), -qmax, qmax),
//                           e' = v - s * float(q); u = 0.5 (nearest) or (x >> 8) * 2^-24 (stochastic),
//                           x the Philox word of the element.
//                         One 32-bit code store per lane, one scale store per group, the residual
//                         (nullable) in place; per block three doubles {sum v^2, sum e'^2, bad
//                         groups} (bad groups left out of the sums), then a one-block finalize,
//                         stream-ordered: stats[4] = {(float)sqrt(sum v^2), (float)sqrt(sum e'^2),
//                         bad groups, 0} as doubles.
//   fd_quant_decode_mean  out = anchor + (sum over the M payloads, in order, of s_c[g] * float(q_c[i]))
//                         * (float)(1 / M), shadow (nullable) = bf16(out); templated on M (1 .. 16).
//
// Payload of n elements at `bits`: n * bits / 32 int32 words of codes (two's complement, element i at
// bit offset i * bits, little-endian), then n / 64 words holding the scales' fp32 bit patterns.
// The stochastic stream: Philox4x32-10 with key (seed_lo ^ 0x51554e54, seed_hi) and counter
// (j lo, j hi, round, client), j = first * 16 + (float4 index); word c of the block belongs to
// component c.  `first` is the index of the tensor's first group in the stream, so a slice encodes
// like the same range of the whole.
//
// Every fp32 operation is rounded on its own (fp contract off).  No atomics: every output word is
// written by exactly one plain store on every launch.
#include "common.h"
#include "philox.h"

#include <cmath>
#include <utility>

namespace {

constexpr int QZ_MAX_M = 16;
constexpr uint32_t QZ_KEY_TAG = 0x51554e54u;  // "QUNT": apart from the privacy noise of the same seed

struct QuantStream {
  uint32_t key_lo, key_hi, round, client;
};

struct DecodeArgs {
  const int32_t* src[QZ_MAX_M];
  const float* anchor;
  float* out;
  bf16_t* shadow;  // nullable
  long long items;       // lanes' work items: n * bits / 32
  long long code_words;  // = items
  float inv;
};

DEV double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <int BITS, bool STOCH>
__global__ __launch_bounds__(256) void quant_encode_kernel(const float* __restrict__ w,
                                                            const float* __restrict__ anchor,
                                                            float* __restrict__ residual,
                                                            int32_t* __restrict__ payload,
                                                            double* __restrict__ partial, QuantStream qs,
                                                            long long first16, long long items) {
#pragma clang fp contract(off)
  constexpr int PER = 32 / BITS;    // elements of a lane
  constexpr int V4 = PER / 4;       // float4 of a lane
  constexpr int LANES = 64 / PER;   // lanes of a group
  constexpr float QMAX = BITS == 8 ? 127.f : 7.f;
  double sum_v = 0.0, sum_e = 0.0;
  int bad = 0;
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < items; i += (long long)gridDim.x * 256) {
    float v[PER];
#pragma unroll
    for (int k = 0; k < V4; ++k) {
      const float4 x = reinterpret_cast<const float4*>(w)[i * V4 + k];
      const float4 a = reinterpret_cast<const float4*>(anchor)[i * V4 + k];
      v[4 * k + 0] = x.x - a.x;
      v[4 * k + 1] = x.y - a.y;
      v[4 * k + 2] = x.z - a.z;
      v[4 * k + 3] = x.w - a.w;
      if (residual) {
        const float4 e = reinterpret_cast<const float4*>(residual)[i * V4 + k];
        v[4 * k + 0] = v[4 * k + 0] + e.x;
        v[4 * k + 1] = v[4 * k + 1] + e.y;
        v[4 * k + 2] = v[4 * k + 2] + e.z;
        v[4 * k + 3] = v[4 * k + 3] + e.w;
      }
    }
    uint32_t m = 0;
#pragma unroll
    for (int e = 0; e < PER; ++e) m = max(m, __float_as_uint(v[e]) & 0x7fffffffu);
#pragma unroll
    for (int o = 1; o < LANES; o <<= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o, 64));
    const float amax = __uint_as_float(m);
    const bool isbad = m >= 0x7f800000u;  // an inf or a NaN in the group
    const float inv = QMAX / amax;
    const bool empty = isbad || m == 0u || !(fabsf(inv) <= 3.402823466e+38f);
    const float s = empty ? 0.f : amax / QMAX;
    uint32_t word = 0;
    float err[PER];
    if (empty) {
#pragma unroll
      for (int e = 0; e < PER; ++e) err[e] = isbad ? 0.f : v[e];
    } else {
#pragma unroll
      for (int k = 0; k < V4; ++k) {
        float u[4] = {0.5f, 0.5f, 0.5f, 0.5f};
        if (STOCH) {
          const unsigned long long j = (unsigned long long)(first16 + i * V4 + k);
          const Philox4 x = philox4x32_10((uint32_t)j, (uint32_t)(j >> 32), qs.round, qs.client, qs.key_lo, qs.key_hi);
          u[0] = (float)(x.x0 >> 8) * 0x1p-24f;
          u[1] = (float)(x.x1 >> 8) * 0x1p-24f;
          u[2] = (float)(x.x2 >> 8) * 0x1p-24f;
          u[3] = (float)(x.x3 >> 8) * 0x1p-24f;
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int e = 4 * k + c;
          const float t = v[e] * inv;
          const float f = fminf(fmaxf(floorf(t + u[c]), -QMAX), QMAX);
          const int q = (int)f;
          const float back = s * f;
          err[e] = v[e] - back;
          word |= ((uint32_t)q & ((1u << BITS) - 1u)) << (BITS * e);
        }
      }
    }
    if (!isbad) {
#pragma unroll
      for (int e = 0; e < PER; ++e) {
        const double dv = (double)v[e], de = (double)err[e];
        sum_v = sum_v + dv * dv;
        sum_e = sum_e + de * de;
      }
    }
    payload[i] = (int32_t)word;
    if ((i & (LANES - 1)) == 0) {
      payload[items + i / LANES] = (int32_t)__float_as_uint(s);
      bad += isbad ? 1 : 0;
    }
    if (residual) {
#pragma unroll
      for (int k = 0; k < V4; ++k)
        reinterpret_cast<float4*>(residual)[i * V4 + k] =
            make_float4(err[4 * k + 0], err[4 * k + 1], err[4 * k + 2], err[4 * k + 3]);
    }
  }
  // lanes -> wave (shuffles) -> block (LDS, fixed order): three doubles per block
  __shared__ double red[3][4];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const double t0 = wave_sum_f64(sum_v), t1 = wave_sum_f64(sum_e), t2 = wave_sum_f64((double)bad);
  if (lane == 0) {
    red[0][wave] = t0;
    red[1][wave] = t1;
    red[2][wave] = t2;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int c = threadIdx.x;
    partial[3ll * blockIdx.x + c] = ((red[c][0] + red[c][1]) + red[c][2]) + red[c][3];
  }
}

__global__ __launch_bounds__(256) void quant_finalize_kernel(const double* __restrict__ partial, int grid,
                                                              double* __restrict__ stats) {
#pragma clang fp contract(off)
  double acc[3] = {0.0, 0.0, 0.0};
  for (int i = threadIdx.x; i < grid; i += 256) {
    acc[0] = acc[0] + partial[3ll * i + 0];
    acc[1] = acc[1] + partial[3ll * i + 1];
    acc[2] = acc[2] + partial[3ll * i + 2];
  }
  __shared__ double red[3][4];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const double t0 = wave_sum_f64(acc[0]), t1 = wave_sum_f64(acc[1]), t2 = wave_sum_f64(acc[2]);
  if (lane == 0) {
    red[0][wave] = t0;
    red[1][wave] = t1;
    red[2][wave] = t2;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const double Sv = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
  const double Se = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
  const double nb = ((red[2][0] + red[2][1]) + red[2][2]) + red[2][3];
  stats[0] = (double)(float)sqrt(Sv);
  stats[1] = (double)(float)sqrt(Se);
  stats[2] = nb;
  stats[3] = 0.0;
}

template <int BITS, int M>
__global__ __launch_bounds__(256) void quant_decode_mean_kernel(DecodeArgs a) {
#pragma clang fp contract(off)
  constexpr int PER = 32 / BITS;
  constexpr int V4 = PER / 4;
  constexpr int LANES = 64 / PER;
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < a.items; i += (long long)gridDim.x * 256) {
    uint32_t word[M];
    float s[M];
#pragma unroll
    for (int c = 0; c < M; ++c) {
      word[c] = (uint32_t)a.src[c][i];
      s[c] = __uint_as_float((uint32_t)a.src[c][a.code_words + i / LANES]);
    }
    float acc[PER];
#pragma unroll
    for (int e = 0; e < PER; ++e) acc[e] = 0.f;
#pragma unroll
    for (int c = 0; c < M; ++c) {
#pragma unroll
      for (int e = 0; e < PER; ++e) {
        const int q = (int)(word[c] << (32 - BITS * (e + 1))) >> (32 - BITS);  // sign-extended code e
        const float p = s[c] * (float)q;
        acc[e] = acc[e] + p;
      }
    }
#pragma unroll
    for (int k = 0; k < V4; ++k) {
      const float4 b = reinterpret_cast<const float4*>(a.anchor)[i * V4 + k];
      const float m0 = acc[4 * k + 0] * a.inv, m1 = acc[4 * k + 1] * a.inv;
      const float m2 = acc[4 * k + 2] * a.inv, m3 = acc[4 * k + 3] * a.inv;
      const float4 o = make_float4(b.x + m0, b.y + m1, b.z + m2, b.w + m3);
      reinterpret_cast<float4*>(a.out)[i * V4 + k] = o;
      if (a.shadow) reinterpret_cast<uint2*>(a.shadow)[i * V4 + k] = make_uint2(pack_bf2(o.x, o.y), pack_bf2(o.z, o.w));
    }
  }
}

// One block per 1024 floats, at most 4096: the grid of fd_privacy_grid (n % 64 == 0 keeps the lane
// groups of both widths whole in every sweep: a sweep is a multiple of 256 lanes).
int qz_grid_for(long long n) { return (int)std::min<long long>((n / 4 + 255) / 256, 4096); }

bool qz_overlap(const void* a, long long ab, const void* b, long long bb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + (uintptr_t)bb && b0 < a0 + (uintptr_t)ab;
}

template <int BITS, int M>
bool qz_decode_launch(const DecodeArgs& a, int grid, hipStream_t st) {
  hipLaunchKernelGGL((quant_decode_mean_kernel<BITS, M>), dim3(grid), dim3(256), 0, st, a);
  return true;
}

template <int BITS, int... Ms>  // Ms = M - 1
bool qz_decode_m(int M, const DecodeArgs& a, int grid, hipStream_t st, std::integer_sequence<int, Ms...>) {
  return ((M == Ms + 1 ? qz_decode_launch<BITS, Ms + 1>(a, grid, st) : false) || ...);
}

}  // namespace

extern "C" {

// Blocks of an fd_quant_encode / fd_quant_decode_mean launch over n floats (encode's partial buffer
// holds three doubles per block).
int fd_quant_grid(long long n) { return n > 0 ? qz_grid_for(n) : 0; }

// int32 words of the payload of n floats at `bits` (8 or 4): codes, then one scale per 64 elements;
// 0 for an n or a width that has no payload.
long long fd_quant_words(long long n, int bits) {
  if (n <= 0 || n % 64 != 0 || (bits != 8 && bits != 4) || n > 0x3fffffffffffffffll / 8) return 0;
  return n * bits / 32 + n / 64;
}

// payload = the codes and scales of (w - anchor) + residual over n floats, residual (nullable) = the
// quantization error, in place; stats[4] (doubles) = {|v|, |e'|, bad groups, 0}; partial holds
// >= 3 * fd_quant_grid(n) doubles and every one of them is overwritten.  n % 64 == 0, bits 8 or 4;
// no two buffers overlap.  `first` is the tensor's first group (64 elements) in the stochastic stream.
int fd_quant_encode(const float* w, const float* anchor, float* residual, int32_t* payload, double* partial,
                    double* stats, int bits, int stochastic, uint32_t seed_lo, uint32_t seed_hi, long long round,
                    long long client, long long first, long long n, hipStream_t st) {
  if (n <= 0 || n % 64 != 0 || n > 0x3fffffffffffffffll / 8) return 1;
  if (!w || !anchor || !payload || !partial || !stats) return 2;
  if (bits != 8 && bits != 4) return 3;
  const long long words = fd_quant_words(n, bits);
  const void* bufs[4] = {w, anchor, residual, payload};
  const long long bytes[4] = {n * 4, n * 4, n * 4, words * 4};
  for (int i = 0; i < 4; ++i)
    for (int j = i + 1; j < 4; ++j)
      if (bufs[i] && bufs[j] && qz_overlap(bufs[i], bytes[i], bufs[j], bytes[j])) return 5;
  if (round < 0 || round > 0xffffffffll) return 6;
  if (client < 0 || client > 0xffffffffll) return 7;
  if (first < 0 || first > (0x7fffffffffffffffll - n / 4) / 16) return 8;
  const QuantStream qs{seed_lo ^ QZ_KEY_TAG, seed_hi, (uint32_t)round, (uint32_t)client};
  const int grid = qz_grid_for(n);
  const long long items = n * bits / 32, first16 = first * 16;
  const dim3 g(grid), b(256);
  if (bits == 8) {
    if (stochastic)
      hipLaunchKernelGGL((quant_encode_kernel<8, true>), g, b, 0, st, w, anchor, residual, payload, partial, qs, first16, items);
    else
      hipLaunchKernelGGL((quant_encode_kernel<8, false>), g, b, 0, st, w, anchor, residual, payload, partial, qs, first16, items);
  } else {
    if (stochastic)
      hipLaunchKernelGGL((quant_encode_kernel<4, true>), g, b, 0, st, w, anchor, residual, payload, partial, qs, first16, items);
    else
      hipLaunchKernelGGL((quant_encode_kernel<4, false>), g, b, 0, st, w, anchor, residual, payload, partial, qs, first16, items);
  }
  hipLaunchKernelGGL(quant_finalize_kernel, dim3(1), dim3(256), 0, st, (const double*)partial, grid, stats);
  return 0;
}

// out = anchor + mean of the M decoded payloads (in the given order) over n floats, shadow
// (nullable) = bf16(out).  1 <= M <= 16, n % 64 == 0, bits 8 or 4; out and shadow overlap no input.
int fd_quant_decode_mean(const int32_t* const* src, int M, const float* anchor, float* out, void* shadow, int bits,
                         long long n, hipStream_t st) {
  if (n <= 0 || n % 64 != 0 || n > 0x3fffffffffffffffll / 8) return 1;
  if (M < 1 || M > QZ_MAX_M) return 2;
  if (bits != 8 && bits != 4) return 3;
  if (!src || !anchor || !out) return 4;
  const long long words = fd_quant_words(n, bits);
  if (qz_overlap(out, n * 4, anchor, n * 4)) return 5;
  if (shadow && (qz_overlap(shadow, n * 2, anchor, n * 4) || qz_overlap(shadow, n * 2, out, n * 4))) return 5;
  DecodeArgs a{};
  for (int s = 0; s < M; ++s) {
    if (!src[s]) return 4;
    if (qz_overlap(src[s], words * 4, out, n * 4) || (shadow && qz_overlap(src[s], words * 4, shadow, n * 2))) return 5;
    a.src[s] = src[s];
  }
  a.anchor = anchor;
  a.out = out;
  a.shadow = (bf16_t*)shadow;
  a.items = n * bits / 32;
  a.code_words = a.items;
  a.inv = (float)(1.0 / (double)M);
  const int grid = qz_grid_for(n);
  const bool ok = bits == 8 ? qz_decode_m<8>(M, a, grid, st, std::make_integer_sequence<int, QZ_MAX_M>{})
                            : qz_decode_m<4>(M, a, grid, st, std::make_integer_sequence<int, QZ_MAX_M>{});
  return ok ? 0 : 2;
}

}  // extern "C"
