// Secure aggregation for the federated exchange (Bonawitz et al., "Practical Secure Aggregation for
// Privacy-Preserving Machine Learning", CCS 2017): a client's round update w - anchor leaves as 32-bit
// fixed point under the sum of one ChaCha stream per live partner, added with opposite signs by the
// two ends of a pair, so the streams cancel in the sum of the payloads mod 2^32 and nowhere else
// (gfx950).  parallel/secagg.py holds the specification (torch_encode, torch_mask, torch_unmask_mean_);
// the kernels equal it bit for bit.
//
//   fd_secagg_stream       out[i] = the generator's word of element 16 * first_block + i for one key
//                          and one nonce: the generator alone, through the device function the mask
//                          pass calls.
//   fd_secagg_mask         one pass.  Per element, every fp32 operation rounded on its own:
//                            d = w - a;  t = d * 2^f;  r = rint(t) (ties to even)
//                            d not finite:  q = 0, counted in bad_elems
//                            |r| >= 2^27:   q = +-(2^27 - 1), counted in clamped
//                            otherwise      q = int32(r)
//                            y = uint32(q) + sum over the P partners of +-word_p(element)  (mod 2^32)
//                          and 16 more words, the check block: q = 1 under the next block of the same
//                          streams.  One 128-bit store per lane; per block four doubles {sum d^2,
//                          sum (d - float(q) 2^-f)^2, clamped, bad} (bad elements left out of the
//                          sums), then a one-block finalize, stream-ordered: stats[4] = {(float)sqrt,
//                          (float)sqrt, clamped, bad} as doubles.  P = 0 is the plain quantizer.
//   fd_secagg_unmask_mean  s = int32(sum of the M payloads mod 2^32); acc = float(s);
//                          out = anchor + (acc * 2^-f) * (float)(1 / M), shadow (nullable) = bf16(out);
//                          templated on M (1 .. 16).
//
// The generator: the ChaCha block function (chacha.h) with the partner's 8 key words, the 32-bit
// block counter first_block + (element / 16) and the nonce (round, 0, 0); a lane is one float4 and a
// quad of lanes one block, element e of the block taking RFC word 4 * (e % 4) + e / 4.  n % 16 == 0
// and a sweep of a multiple of 256 lanes keep every quad whole in every iteration.  With M - 1
// streams per element the mask pass is integer-ALU-bound, not bandwidth-bound: the keys sit in LDS,
// two partners' blocks run side by side (at two the compiler folds every quad rotation into the add or
// xor that reads it; at four it keeps them as moves), and the round count is a template parameter.
//
// Every fp32 operation is rounded on its own (fp contract off).  No atomics: every output word is
// written by exactly one plain store on every launch.
#include "chacha.h"
#include "common.h"

#include <cmath>
#include <utility>

namespace {

constexpr int SA_MAX_M = 16;
constexpr int SA_MAX_P = SA_MAX_M - 1;
constexpr int SA_GRID_CAP = 2048;  // one resident round of 256-lane blocks at 8 waves per SIMD
constexpr int SA_QMAX = (1 << 27) - 1;
constexpr int SA_SIDE = 2;  // partners whose blocks go through the rounds side by side

struct UnmaskArgs {
  const int32_t* src[SA_MAX_M];
  const float* anchor;
  float* out;
  bf16_t* shadow;  // nullable
  long long n4;
  float inv_scale, inv;
};

DEV double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// the fixed-point code of one element and its part in the block's four sums
DEV int sa_quantize(float x, float a, float scale, float inv_scale, double& sum_d, double& sum_e, int& clamped,
                    int& bad) {
#pragma clang fp contract(off)
  const float d = x - a;
  if (!(fabsf(d) <= 3.402823466e+38f)) {  // inf or NaN
    bad += 1;
    return 0;
  }
  const float t = d * scale;
  const float r = rintf(t);
  int q;
  if (!(fabsf(r) < 134217728.f)) {  // 2^27, or a t that overflowed
    q = r < 0.f ? -SA_QMAX : SA_QMAX;
    clamped += 1;
  } else {
    q = (int)r;
  }
  const float back = (float)q * inv_scale;
  const float e = d - back;
  const double dd = (double)d, de = (double)e;
  sum_d = sum_d + dd * dd;
  sum_e = sum_e + de * de;
  return q;
}

DEV void sa_add(uint4& acc, const uint4& x, bool neg) {
  acc.x = neg ? acc.x - x.x : acc.x + x.x;
  acc.y = neg ? acc.y - x.y : acc.y + x.y;
  acc.z = neg ? acc.z - x.z : acc.z + x.z;
  acc.w = neg ? acc.w - x.w : acc.w + x.w;
}

// acc += the signed words of partners [0, P) for this lane's float4 of block `counter`; skey holds the
// partners' keys (8 words each) in LDS
template <int ROUNDS>
DEV void sa_mask_words(uint4& acc, const uint32_t* skey, int P, uint32_t signs, int col, uint32_t d0) {
  int p = 0;
  for (; p + SA_SIDE <= P; p += SA_SIDE) {
    uint32_t kb[SA_SIDE], kc[SA_SIDE];
    uint4 x[SA_SIDE];
#pragma unroll
    for (int u = 0; u < SA_SIDE; ++u) {
      kb[u] = skey[(p + u) * 8 + col];
      kc[u] = skey[(p + u) * 8 + 4 + col];
    }
    chacha_columns<ROUNDS, SA_SIDE>(col, kb, kc, d0, x);
#pragma unroll
    for (int u = 0; u < SA_SIDE; ++u) sa_add(acc, x[u], (signs >> (p + u)) & 1u);
  }
  for (; p < P; ++p) {
    const uint32_t kb[1] = {skey[p * 8 + col]}, kc[1] = {skey[p * 8 + 4 + col]};
    uint4 x[1];
    chacha_columns<ROUNDS, 1>(col, kb, kc, d0, x);
    sa_add(acc, x[0], (signs >> p) & 1u);
  }
}

template <int ROUNDS>
__global__ __launch_bounds__(256) void secagg_mask_kernel(const float* __restrict__ w, const float* __restrict__ anchor,
                                                           const uint32_t* __restrict__ keys, int P, uint32_t signs,
                                                           uint32_t nonce0, int32_t* __restrict__ payload,
                                                           double* __restrict__ partial, float scale, float inv_scale,
                                                           unsigned long long first_block, long long n4) {
  __shared__ uint32_t skey[SA_MAX_P * 8];
  __shared__ double red[4][4];
  for (int t = threadIdx.x; t < P * 8; t += 256) skey[t] = keys[t];
  __syncthreads();
  const int col = threadIdx.x & 3;  // (a sweep is a multiple of 256 lanes: i & 3 == col throughout)
  const uint32_t d_rest = col == 1 ? nonce0 : 0u;
  double sum_d = 0.0, sum_e = 0.0;
  int clamped = 0, bad = 0;
  const long long items = n4 + 4;  // the check block: four float4 behind the tensor
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < items; i += (long long)gridDim.x * 256) {
    uint4 acc;
    if (i < n4) {
      const float4 x = reinterpret_cast<const float4*>(w)[i];
      const float4 a = reinterpret_cast<const float4*>(anchor)[i];
      acc.x = (uint32_t)sa_quantize(x.x, a.x, scale, inv_scale, sum_d, sum_e, clamped, bad);
      acc.y = (uint32_t)sa_quantize(x.y, a.y, scale, inv_scale, sum_d, sum_e, clamped, bad);
      acc.z = (uint32_t)sa_quantize(x.z, a.z, scale, inv_scale, sum_d, sum_e, clamped, bad);
      acc.w = (uint32_t)sa_quantize(x.w, a.w, scale, inv_scale, sum_d, sum_e, clamped, bad);
    } else {
      acc = make_uint4(1u, 1u, 1u, 1u);
    }
    const uint32_t counter = (uint32_t)(first_block + (unsigned long long)(i >> 2));
    sa_mask_words<ROUNDS>(acc, skey, P, signs, col, col == 0 ? counter : d_rest);
    reinterpret_cast<uint4*>(payload)[i] = acc;
  }
  // lanes -> wave (shuffles) -> block (LDS, fixed order): four doubles per block
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const double t0 = wave_sum_f64(sum_d), t1 = wave_sum_f64(sum_e);
  const double t2 = wave_sum_f64((double)clamped), t3 = wave_sum_f64((double)bad);
  if (lane == 0) {
    red[0][wave] = t0;
    red[1][wave] = t1;
    red[2][wave] = t2;
    red[3][wave] = t3;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    const int c = threadIdx.x;
    partial[4ll * blockIdx.x + c] = ((red[c][0] + red[c][1]) + red[c][2]) + red[c][3];
  }
}

__global__ __launch_bounds__(256) void secagg_finalize_kernel(const double* __restrict__ partial, int grid,
                                                               double* __restrict__ stats) {
#pragma clang fp contract(off)
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int i = threadIdx.x; i < grid; i += 256) {
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] = acc[c] + partial[4ll * i + c];
  }
  __shared__ double red[4][4];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double t[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) t[c] = wave_sum_f64(acc[c]);
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < 4; ++c) red[c][wave] = t[c];
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double S[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) S[c] = ((red[c][0] + red[c][1]) + red[c][2]) + red[c][3];
  stats[0] = (double)(float)sqrt(S[0]);
  stats[1] = (double)(float)sqrt(S[1]);
  stats[2] = S[2];
  stats[3] = S[3];
}

template <int ROUNDS>
__global__ __launch_bounds__(256) void secagg_stream_kernel(int32_t* __restrict__ out, const uint32_t* __restrict__ key,
                                                             uint32_t nonce0, uint32_t nonce1, uint32_t nonce2,
                                                             unsigned long long first_block, long long n4) {
  __shared__ uint32_t skey[8];
  if (threadIdx.x < 8) skey[threadIdx.x] = key[threadIdx.x];
  __syncthreads();
  const int col = threadIdx.x & 3;
  const uint32_t d_rest = col == 1 ? nonce0 : col == 2 ? nonce1 : nonce2;
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
    uint4 acc = make_uint4(0u, 0u, 0u, 0u);
    const uint32_t counter = (uint32_t)(first_block + (unsigned long long)(i >> 2));
    sa_mask_words<ROUNDS>(acc, skey, 1, 0u, col, col == 0 ? counter : d_rest);
    reinterpret_cast<uint4*>(out)[i] = acc;
  }
}

template <int M>
__global__ __launch_bounds__(256) void secagg_unmask_mean_kernel(UnmaskArgs a) {
#pragma clang fp contract(off)
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < a.n4; i += (long long)gridDim.x * 256) {
    uint4 s = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
    for (int c = 0; c < M; ++c) {
      const uint4 y = reinterpret_cast<const uint4*>(a.src[c])[i];
      s.x += y.x;
      s.y += y.y;
      s.z += y.z;
      s.w += y.w;
    }
    const float4 b = reinterpret_cast<const float4*>(a.anchor)[i];
    const float u0 = (float)(int)s.x * a.inv_scale, u1 = (float)(int)s.y * a.inv_scale;
    const float u2 = (float)(int)s.z * a.inv_scale, u3 = (float)(int)s.w * a.inv_scale;
    const float m0 = u0 * a.inv, m1 = u1 * a.inv, m2 = u2 * a.inv, m3 = u3 * a.inv;
    const float4 o = make_float4(b.x + m0, b.y + m1, b.z + m2, b.w + m3);
    reinterpret_cast<float4*>(a.out)[i] = o;
    if (a.shadow) reinterpret_cast<uint2*>(a.shadow)[i] = make_uint2(pack_bf2(o.x, o.y), pack_bf2(o.z, o.w));
  }
}

int sa_grid_for(long long items) { return (int)std::min<long long>((items + 255) / 256, SA_GRID_CAP); }

bool sa_overlap(const void* a, long long ab, const void* b, long long bb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + (uintptr_t)bb && b0 < a0 + (uintptr_t)ab;
}

bool sa_aligned(const void* p) { return ((uintptr_t)p & 15u) == 0; }

bool sa_n_ok(long long n) { return n > 0 && n % 16 == 0 && n <= 0x3fffffffffffffffll / 8; }

// the block counters first_block .. first_block + n / 16 - 1 + extra (extra = 1: the check block) fit 32 bits
bool sa_blocks_ok(long long first_block, long long n, int extra) {
  return first_block >= 0 && first_block <= 0x100000000ll && first_block + n / 16 + extra <= 0x100000000ll;
}

template <int M>
bool sa_unmask_launch(const UnmaskArgs& a, int grid, hipStream_t st) {
  hipLaunchKernelGGL((secagg_unmask_mean_kernel<M>), dim3(grid), dim3(256), 0, st, a);
  return true;
}

template <int... Ms>  // Ms = M - 1
bool sa_unmask_m(int M, const UnmaskArgs& a, int grid, hipStream_t st, std::integer_sequence<int, Ms...>) {
  return ((M == Ms + 1 ? sa_unmask_launch<Ms + 1>(a, grid, st) : false) || ...);
}

}  // namespace

extern "C" {

// Blocks of an fd_secagg_mask launch over n floats (its partial buffer holds four doubles per block);
// fd_secagg_stream and fd_secagg_unmask_mean launch no more.
int fd_secagg_grid(long long n) { return n > 0 ? sa_grid_for(n / 4 + 4) : 0; }

// int32 words of the payload of n floats: one per element, then the 16 of the check block; 0 for an n
// that has no payload.
long long fd_secagg_words(long long n) { return sa_n_ok(n) ? n + 16 : 0; }

// out[i] = the generator's word of element 16 * first_block + i over n words, for the key (8 words on
// the device) and the nonce (three words); rounds 8, 12 or 20; n % 16 == 0, first_block + n / 16 <= 2^32.
int fd_secagg_stream(int32_t* out, const uint32_t* key, uint32_t nonce0, uint32_t nonce1, uint32_t nonce2, int rounds,
                     long long first_block, long long n, hipStream_t st) {
  if (!sa_n_ok(n)) return 1;
  if (!out || !key || !sa_aligned(out)) return 2;
  if (rounds != 8 && rounds != 12 && rounds != 20) return 3;
  if (!sa_blocks_ok(first_block, n, 0)) return 8;
  if (sa_overlap(out, n * 4, key, 32)) return 5;
  const dim3 g(sa_grid_for(n / 4)), b(256);
  const unsigned long long fb = (unsigned long long)first_block;
  if (rounds == 8)
    hipLaunchKernelGGL((secagg_stream_kernel<8>), g, b, 0, st, out, key, nonce0, nonce1, nonce2, fb, n / 4);
  else if (rounds == 12)
    hipLaunchKernelGGL((secagg_stream_kernel<12>), g, b, 0, st, out, key, nonce0, nonce1, nonce2, fb, n / 4);
  else
    hipLaunchKernelGGL((secagg_stream_kernel<20>), g, b, 0, st, out, key, nonce0, nonce1, nonce2, fb, n / 4);
  return 0;
}

// payload (n + 16 words) = the masked fixed-point codes of w - anchor over n floats and the check
// block; keys holds P x 8 words on the device (nullable at P = 0), bit p of signs set: partner p's
// stream is subtracted.  stats[4] (doubles) = {|d|, |d - float(q) 2^-f|, clamped, bad}; partial holds
// >= 4 * fd_secagg_grid(n) doubles and every one of them is overwritten.  n % 16 == 0, 0 <= P <= 15,
// 8 <= frac_bits <= 30, rounds 8, 12 or 20, first_block + n / 16 + 1 <= 2^32; no two buffers overlap.
int fd_secagg_mask(const float* w, const float* anchor, const uint32_t* keys, int P, uint32_t signs, int32_t* payload,
                   double* partial, double* stats, int frac_bits, int rounds, long long round, long long first_block,
                   long long n, hipStream_t st) {
  if (!sa_n_ok(n)) return 1;
  if (!w || !anchor || !payload || !partial || !stats || (P > 0 && !keys)) return 2;
  if (!sa_aligned(w) || !sa_aligned(anchor) || !sa_aligned(payload)) return 2;
  if (rounds != 8 && rounds != 12 && rounds != 20) return 3;
  if (P < 0 || P > SA_MAX_P || (signs >> P) != 0u) return 4;
  if (frac_bits < 8 || frac_bits > 30) return 6;
  if (round < 0 || round > 0xffffffffll) return 7;
  if (!sa_blocks_ok(first_block, n, 1)) return 8;
  const int grid = fd_secagg_grid(n);
  const void* bufs[6] = {w, anchor, payload, partial, stats, keys};
  const long long bytes[6] = {n * 4, n * 4, (n + 16) * 4, 32ll * grid, 32, 32ll * P};
  for (int i = 0; i < 6; ++i)
    for (int j = i + 1; j < 6; ++j)
      if (bufs[i] && bufs[j] && bytes[i] && bytes[j] && sa_overlap(bufs[i], bytes[i], bufs[j], bytes[j])) return 5;
  const float scale = ldexpf(1.f, frac_bits), inv_scale = ldexpf(1.f, -frac_bits);
  const dim3 g(grid), b(256);
  const unsigned long long fb = (unsigned long long)first_block;
  const uint32_t n0 = (uint32_t)round;
  if (rounds == 8)
    hipLaunchKernelGGL((secagg_mask_kernel<8>), g, b, 0, st, w, anchor, keys, P, signs, n0, payload, partial, scale,
                       inv_scale, fb, n / 4);
  else if (rounds == 12)
    hipLaunchKernelGGL((secagg_mask_kernel<12>), g, b, 0, st, w, anchor, keys, P, signs, n0, payload, partial, scale,
                       inv_scale, fb, n / 4);
  else
    hipLaunchKernelGGL((secagg_mask_kernel<20>), g, b, 0, st, w, anchor, keys, P, signs, n0, payload, partial, scale,
                       inv_scale, fb, n / 4);
  hipLaunchKernelGGL(secagg_finalize_kernel, dim3(1), dim3(256), 0, st, (const double*)partial, grid, stats);
  return 0;
}

// out = anchor + the fixed-point mean of the M payloads' modular sum over n floats (the check block is
// not read), shadow (nullable) = bf16(out).  1 <= M <= 16, n % 16 == 0; out and shadow overlap no input.
int fd_secagg_unmask_mean(const int32_t* const* src, int M, const float* anchor, float* out, void* shadow,
                          int frac_bits, long long n, hipStream_t st) {
  if (!sa_n_ok(n)) return 1;
  if (M < 1 || M > SA_MAX_M) return 2;
  if (frac_bits < 8 || frac_bits > 30) return 6;
  if (!src || !anchor || !out) return 4;
  if (!sa_aligned(anchor) || !sa_aligned(out) || (shadow && ((uintptr_t)shadow & 7u))) return 4;
  if (sa_overlap(out, n * 4, anchor, n * 4)) return 5;
  if (shadow && (sa_overlap(shadow, n * 2, anchor, n * 4) || sa_overlap(shadow, n * 2, out, n * 4))) return 5;
  UnmaskArgs a{};
  for (int s = 0; s < M; ++s) {
    if (!src[s] || !sa_aligned(src[s])) return 4;
    if (sa_overlap(src[s], (n + 16) * 4, out, n * 4) || (shadow && sa_overlap(src[s], (n + 16) * 4, shadow, n * 2)))
      return 5;
    a.src[s] = src[s];
  }
  a.anchor = anchor;
  a.out = out;
  a.shadow = (bf16_t*)shadow;
  a.n4 = n / 4;
  a.inv_scale = ldexpf(1.f, -frac_bits);
  a.inv = (float)(1.0 / (double)M);
  return sa_unmask_m(M, a, sa_grid_for(n / 4), st, std::make_integer_sequence<int, SA_MAX_M>{}) ? 0 : 2;
}

}  // extern "C"
