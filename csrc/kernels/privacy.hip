// Client-level differential privacy for the federated exchange (DP-FedAvg: McMahan et al., ICLR
// 2018; Geyer et al., 2017): the L2 norm of a client's round update w - anchor is bounded by clip,
// and Gaussian noise is added, in two bandwidth-bound passes over the fp32 arena (gfx950).
//
//   fd_privacy_norm   (a) per block, the sum of d * d, d = w - anchor: per lane an fp32 running sum
//                     (the four components of a float4 in order, iterations in order), converted to
//                     double, reduced wave -> block in a fixed order, one double per block;
//                     (b) a one-block finalize, stream-ordered after (a): S = the sum of the
//                     partials in double (fixed order), norm = (float)sqrt(S),
//                     stats = {norm, scale, flag, 0}:
//                       flag 0, scale 1            norm <= clip
//                       flag 1, scale clip / norm  norm >  clip   (IEEE fp32 division)
//                       flag 2, scale 0            norm is not finite
//   fd_privacy_apply  in place on w, scale and flag read from stats on the device (no host sync
//                     between the passes).  Per element, every operation rounded on its own:
//                       flag 0: u = w       flag 1: d = w - a; t = scale * d; u = a + t
//                       flag 2: u = a       then, if sigma != 0: u = u + sigma * g(index)
//                     w = u, shadow (nullable) = bf16(u).
//   fd_privacy_gauss  out[i] = g(4 * first4 + i): the generator alone, through the device function
//                     apply calls.
//
// The generator g is counter-based: Philox4x32-10 (Salmon et al., "Parallel Random Numbers: As Easy
// as 1, 2, 3", SC 2011) with key (seed_lo, seed_hi) and counter (j lo, j hi, round, client) for
// float4 index j; its four words make the float4's four Gaussians by two Box-Muller pairs,
//   u1 = ((x0 >> 8) + 1) * 2^-24 in (0, 1],  u2 = (x1 >> 8) * 2^-24 in [0, 1),
//   r = sqrt(-2 ln u1),  g0 = r cos(2 pi u2),  g1 = r sin(2 pi u2);  g2, g3 likewise from x2, x3,
// so a value depends on its global index alone, never on the launch geometry, and
// |g| <= sqrt(48 ln 2) = 5.77.  The 24-bit uniforms are exact in fp32; the angle goes through
// sincospif(2 u2), whose argument is exact too.  parallel/privacy.py mirrors the generator on the
// host (philox4x32_10 bit for bit, torch_gauss in fp64).
//
// No atomics: every output entry is written by exactly one plain store on every launch.
#include "common.h"
#include "philox.h"

#include <cmath>

namespace {

struct PrivacyStream {
  uint32_t seed_lo, seed_hi, round, client;
};

DEV void box_muller(uint32_t xa, uint32_t xb, float& ga, float& gb) {
#pragma clang fp contract(off)
  const float u1 = (float)((xa >> 8) + 1u) * 0x1p-24f;
  const float u2 = (float)(xb >> 8) * 0x1p-24f;
  const float r = sqrtf(-2.0f * logf(u1));
  float s, c;
  sincospif(2.0f * u2, &s, &c);
  ga = r * c;
  gb = r * s;
}

// The four standard Gaussians of float4 index j (elements 4j .. 4j + 3) of stream ps.
DEV float4 privacy_gauss4(long long j, const PrivacyStream& ps) {
  const unsigned long long uj = (unsigned long long)j;
  const Philox4 x = philox4x32_10((uint32_t)uj, (uint32_t)(uj >> 32), ps.round, ps.client, ps.seed_lo, ps.seed_hi);
  float4 g;
  box_muller(x.x0, x.x1, g.x, g.y);
  box_muller(x.x2, x.x3, g.z, g.w);
  return g;
}

DEV double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// lanes -> wave (shuffles) -> block (LDS, fixed order); the block's sum is returned to thread 0
DEV double block_sum_f64(double v) {
  __shared__ double red[4];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const double t = wave_sum_f64(v);
  if (lane == 0) red[wave] = t;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(256) void privacy_norm_kernel(const float* __restrict__ w, const float* __restrict__ anchor,
                                                            double* __restrict__ partial, long long n4) {
#pragma clang fp contract(off)
  float acc = 0.f;
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
    const float4 x = reinterpret_cast<const float4*>(w)[i];
    const float4 a = reinterpret_cast<const float4*>(anchor)[i];
    const float d0 = x.x - a.x, d1 = x.y - a.y, d2 = x.z - a.z, d3 = x.w - a.w;
    acc = acc + d0 * d0;
    acc = acc + d1 * d1;
    acc = acc + d2 * d2;
    acc = acc + d3 * d3;
  }
  const double s = block_sum_f64((double)acc);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void privacy_finalize_kernel(const double* __restrict__ partial, int grid,
                                                                float* __restrict__ stats, float clip) {
#pragma clang fp contract(off)
  double acc = 0.0;
  for (int i = threadIdx.x; i < grid; i += 256) acc = acc + partial[i];
  const double S = block_sum_f64(acc);
  if (threadIdx.x != 0) return;
  const float norm = (float)sqrt(S);
  float scale = 1.f, flag = 0.f;
  if (!(fabsf(norm) <= 3.402823466e+38f)) {  // NaN or inf
    scale = 0.f;
    flag = 2.f;
  } else if (norm > clip) {
    scale = clip / norm;
    flag = 1.f;
  }
  stats[0] = norm;
  stats[1] = scale;
  stats[2] = flag;
  stats[3] = 0.f;
}

__global__ __launch_bounds__(256) void privacy_apply_kernel(float* __restrict__ w, const float* __restrict__ anchor,
                                                             bf16_t* __restrict__ shadow,
                                                             const float* __restrict__ stats, float sigma,
                                                             PrivacyStream ps, long long first4, long long n4) {
#pragma clang fp contract(off)
  const float scale = stats[1];
  const int flag = (int)stats[2];  // uniform over the launch
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
    float4 u;
    if (flag == 0) {
      u = reinterpret_cast<const float4*>(w)[i];  // (not re-rounded through a + (w - a))
    } else if (flag == 1) {
      const float4 x = reinterpret_cast<const float4*>(w)[i];
      const float4 a = reinterpret_cast<const float4*>(anchor)[i];
      const float t0 = scale * (x.x - a.x), t1 = scale * (x.y - a.y);
      const float t2 = scale * (x.z - a.z), t3 = scale * (x.w - a.w);
      u = make_float4(a.x + t0, a.y + t1, a.z + t2, a.w + t3);
    } else {
      u = reinterpret_cast<const float4*>(anchor)[i];  // a diverged client sends a zero update
    }
    if (sigma != 0.f) {
      const float4 g = privacy_gauss4(first4 + i, ps);
      const float s0 = sigma * g.x, s1 = sigma * g.y, s2 = sigma * g.z, s3 = sigma * g.w;
      u = make_float4(u.x + s0, u.y + s1, u.z + s2, u.w + s3);
    }
    reinterpret_cast<float4*>(w)[i] = u;
    if (shadow) reinterpret_cast<uint2*>(shadow)[i] = make_uint2(pack_bf2(u.x, u.y), pack_bf2(u.z, u.w));
  }
}

__global__ __launch_bounds__(256) void privacy_gauss_kernel(float* __restrict__ out, PrivacyStream ps, long long first4,
                                                             long long n4) {
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n4; i += (long long)gridDim.x * 256)
    reinterpret_cast<float4*>(out)[i] = privacy_gauss4(first4 + i, ps);
}

int pv_grid_for(long long n4) { return (int)std::min<long long>((n4 + 255) / 256, 4096); }

bool pv_overlap(const void* a, long long ab, const void* b, long long bb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + (uintptr_t)bb && b0 < a0 + (uintptr_t)ab;
}

// round, client >= 0 and below 2^32 (one counter word each); first4 >= 0 and the last float4 index
// representable
int pv_stream_rc(long long round, long long client, long long first4, long long n4) {
  if (round < 0 || round > 0xffffffffll) return 6;
  if (client < 0 || client > 0xffffffffll) return 7;
  if (first4 < 0 || first4 > 0x7fffffffffffffffll - n4) return 8;
  return 0;
}

}  // namespace

extern "C" {

// Blocks of an fd_privacy_norm / apply / gauss launch over n floats (the norm's partial buffer holds
// one double per block): the grid of fd_robust_agg and fd_server_opt.
int fd_privacy_grid(long long n) { return n > 0 ? pv_grid_for(n / 4) : 0; }

// stats[4] = {|w - anchor|, scale, flag, 0} over n floats; partial holds >= fd_privacy_grid(n)
// doubles and every one of them is overwritten.  n % 4 == 0, clip finite and > 0, anchor apart from w.
int fd_privacy_norm(const float* w, const float* anchor, double* partial, float* stats, float clip, long long n,
                    hipStream_t st) {
  if (n <= 0 || n % 4 != 0) return 1;
  if (!w || !anchor || !partial || !stats) return 2;
  if (!std::isfinite(clip) || !(clip > 0.f)) return 3;
  if (pv_overlap(w, n * 4, anchor, n * 4)) return 5;
  const int grid = pv_grid_for(n / 4);
  hipLaunchKernelGGL(privacy_norm_kernel, dim3(grid), dim3(256), 0, st, w, anchor, partial, n / 4);
  hipLaunchKernelGGL(privacy_finalize_kernel, dim3(1), dim3(256), 0, st, (const double*)partial, grid, stats, clip);
  return 0;
}

// w = clip(w; anchor, stats) + sigma * g over n floats, shadow (nullable) = bf16(w); element i has
// the global index 4 * first4 + i.  anchor must not overlap w, shadow neither of them.
int fd_privacy_apply(float* w, const float* anchor, void* shadow, const float* stats, float sigma, uint32_t seed_lo,
                     uint32_t seed_hi, long long round, long long client, long long first4, long long n,
                     hipStream_t st) {
  if (n <= 0 || n % 4 != 0) return 1;
  if (!w || !anchor || !stats) return 2;
  if (!std::isfinite(sigma) || !(sigma >= 0.f)) return 4;
  if (pv_overlap(w, n * 4, anchor, n * 4)) return 5;
  if (shadow && (pv_overlap(shadow, n * 2, w, n * 4) || pv_overlap(shadow, n * 2, anchor, n * 4))) return 5;
  if (const int rc = pv_stream_rc(round, client, first4, n / 4)) return rc;
  const PrivacyStream ps{seed_lo, seed_hi, (uint32_t)round, (uint32_t)client};
  hipLaunchKernelGGL(privacy_apply_kernel, dim3(pv_grid_for(n / 4)), dim3(256), 0, st, w, anchor, (bf16_t*)shadow,
                     stats, sigma, ps, first4, n / 4);
  return 0;
}

// out[i] = g(4 * first4 + i) over n floats.
int fd_privacy_gauss(float* out, uint32_t seed_lo, uint32_t seed_hi, long long round, long long client,
                     long long first4, long long n, hipStream_t st) {
  if (n <= 0 || n % 4 != 0) return 1;
  if (!out) return 2;
  if (const int rc = pv_stream_rc(round, client, first4, n / 4)) return rc;
  const PrivacyStream ps{seed_lo, seed_hi, (uint32_t)round, (uint32_t)client};
  hipLaunchKernelGGL(privacy_gauss_kernel, dim3(pv_grid_for(n / 4)), dim3(256), 0, st, out, ps, first4, n / 4);
  return 0;
}

}  // extern "C"
