// Top-k sparsified update exchange (Aji & Heafield, EMNLP 2017; Deep Gradient Compression, Lin et
// al., ICLR 2018; error feedback: Stich et al., NeurIPS 2018): a client sends the k entries of its
// round update v = (w - anchor) + e with the largest magnitudes and keeps the rest as its residual;
// the mean of M such sparse payloads is scattered onto the anchor in one dense pass (gfx950).
// parallel/compress.py holds the specification (torch_topk_encode_, torch_topk_decode_mean_); the
// kernels equal it bit for bit.
//
// Key of element i: the 31-bit pattern of |v_i|.  A key >= 0x7f800000 (inf, NaN) is *bad*: no
// candidate, never sent, residual +0.  The sent set is the k_eff = min(k, n - bad) candidates with
// the largest keys, ties broken by the lower index.
//
//   fd_topk_encode   a fixed sequence of stream-ordered launches, nothing read back by the host:
//     clear          the three histograms and the select state
//     hist<0>        v = (w - anchor) + e, stored once (into the residual, or into `work` without
//                    one) so every later pass reads one stream; histogram of key >> 20 (2048 bins;
//                    the bad keys are exactly bins 2040 .. 2047)
//     select<0>      one block: bad = the top eight bins, k_eff, the bin that holds the k_eff-th
//                    largest key and the rank that remains inside it
//     hist<1>, select<1>, hist<2>, select<2>
//                    the same over bits 19 .. 10 and 9 .. 0 of the keys that match the prefix so
//                    far (1024 bins each): after the third the threshold key T is exact and the
//                    remaining rank is the tie budget -- how many keys == T are sent
//     count          per chunk of 4096 elements: keys > T, keys == T
//     scan           one block: exclusive scan of both over the chunks; writes the payload's offsets
//     emit           recomputes the flags; an element with key == T is sent while its rank among
//                    all such elements (by index) is below the budget; ranks inside the chunk come
//                    from wave scans + 16 LDS words; writes values, uint16 local indices, the
//                    residual and per-block fp64 sums of squares; zero-fills entries k_eff .. k
//     finalize       one block: stats[8] (doubles) = {|v|, |e'|, bad, sent, threshold, 0, 0, 0}
//   fd_topk_decode_mean   a block owns whole chunks: a 4096-float accumulator in LDS, the M payloads'
//                    entries of the chunk added in payload order (a barrier between payloads), then
//                    out = anchor + acc * (float)(1 / M), shadow = bf16(out).  Offsets are clamped
//                    into [0, k] and made ascending, a local index beyond the chunk is dropped: no
//                    payload content makes it read or write out of bounds.
//
// Payload of n elements with k entries (C = ceil(n / 4096) chunks), int32 words:
//   [0, C]               off[b] = sent entries in chunks < b (off[C] = k_eff)
//   [C + 1, C + 1 + k)   fp32 bit patterns of v at the sent elements, ascending index; 0 from k_eff on
//   then ceil(k / 2)     local indices (i mod 4096) as uint16, entry j in the low (j even) or high
//                        half of word j / 2; unused halves 0
//
// Histogram contention: update magnitudes crowd into a few exponent bins (and untouched embedding
// rows are exactly zero), so a lane-per-element LDS atomic would serialise.  hist_add aggregates
// equal bins inside the wave (ballot of the lanes that share the first live lane's bin, one add of
// the popcount) for up to four distinct bins, then lets the few lanes left add singly.
//
// Determinism: no float atomics.  Integer atomics only into histograms (sums: order-free).  Every
// payload word, residual element and stats word is written by plain stores on every launch.
#include "common.h"

#include <cmath>
#include <utility>

namespace {

constexpr int TK_MAX_M = 16;
constexpr int TK_CHUNK = 4096;
constexpr int TK_GRID_CAP = 1024;
constexpr uint32_t TK_BAD = 0x7f800000u;   // keys from here on: inf / NaN
constexpr uint32_t TK_NONE = 0xffffffffu;  // prefix / threshold when nothing is sent
constexpr int TK_H0 = 2048, TK_H1 = 1024, TK_H2 = 1024;
constexpr int TK_STATE = 16;               // uint32 words of select state
// state words
constexpr int ST_PREFIX = 0, ST_RANK = 1, ST_BAD = 2, ST_KEFF = 3, ST_T = 4, ST_BUDGET = 5;

struct TopkWork {
  float* v;            // n floats (used without a residual)
  uint32_t* hist;      // TK_H0 + TK_H1 + TK_H2, then TK_STATE words of state
  uint32_t* state;
  uint32_t* cnt;       // [C][2] keys > T, keys == T
  uint32_t* offs;      // [C][2] their exclusive scans
  double* partial;     // [grid][2]
};

long long tk_chunks(long long n) { return (n + TK_CHUNK - 1) / TK_CHUNK; }
int tk_grid_for(long long n) { return (int)std::min<long long>(tk_chunks(n), TK_GRID_CAP); }

long long tk_work_bytes(long long n) {
  const long long C = tk_chunks(n);
  return n * 4 + (TK_H0 + TK_H1 + TK_H2 + TK_STATE) * 4ll + C * 16 + tk_grid_for(n) * 16ll;
}

TopkWork tk_carve(void* work, long long n) {
  const long long C = tk_chunks(n);
  char* p = (char*)work;
  TopkWork w;
  w.v = (float*)p;
  p += n * 4;
  w.hist = (uint32_t*)p;
  w.state = w.hist + TK_H0 + TK_H1 + TK_H2;
  p += (TK_H0 + TK_H1 + TK_H2 + TK_STATE) * 4ll;
  w.cnt = (uint32_t*)p;
  p += C * 8;
  w.offs = (uint32_t*)p;
  p += C * 8;
  w.partial = (double*)p;  // n * 4 and every size above are multiples of 8
  return w;
}

// (xor shuffles by ds_bpermute on the lane index: __shfl_xor's range checks would sit in SGPRs as
// wave predicates for the whole kernel)
DEV uint32_t tk_xor_u32(uint32_t v, int o) {
  const int lane = (int)__lane_id();
  return (uint32_t)__builtin_amdgcn_ds_bpermute((lane ^ o) << 2, (int)v);
}

DEV double tk_wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    const unsigned long long w = (unsigned long long)tk_xor_u32((uint32_t)u, o) |
                                 ((unsigned long long)tk_xor_u32((uint32_t)(u >> 32), o) << 32);
    v += __longlong_as_double((long long)w);
  }
  return v;
}

DEV uint32_t tk_wave_sum_u32(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += tk_xor_u32(v, o);
  return v;
}

// all ones when a < b (both below 2^31): a lane mask kept in a VGPR, not as a wave predicate in SGPRs
DEV uint32_t tk_lt_mask(int a, int b) {
  uint32_t m = (uint32_t)((a - b) >> 31);
  asm volatile("" : "+v"(m));  // (opaque: otherwise the compiler turns it back into a compare)
  return m;
}

// inclusive scan over the wave's lanes
DEV uint32_t tk_wave_scan_u32(uint32_t v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int src = lane - o;  // lanes below o read lane 0 and mask its value out
    const uint32_t u = (uint32_t)__builtin_amdgcn_ds_bpermute((src & ~(src >> 31)) << 2, (int)v);
    v += u & tk_lt_mask(o - 1, lane);
  }
  return v;
}

// One count into h[bin] for every lane with `active`, equal bins aggregated inside the wave.  Called
// by all 64 lanes together.
DEV void hist_add(uint32_t* h, uint32_t bin, bool active, int lane) {
#pragma unroll 1
  for (int it = 0; it < 4; ++it) {
    const unsigned long long live = __ballot(active);
    if (live == 0ull) return;
    const int leader = __ffsll((long long)live) - 1;
    const uint32_t b = (uint32_t)__shfl((int)bin, leader, 64);
    const bool same = active && bin == b;
    const unsigned long long m = __ballot(same);
    if (lane == leader) atomicAdd(&h[b], (uint32_t)__popcll(m));
    active = active && !same;
  }
  if (active) atomicAdd(&h[bin], 1u);
}

// LEVEL 0: v = (w - anchor) + e -> vbuf, bins key >> 20.  LEVEL 1 / 2: keys whose bits above the
// level's ten match the prefix, bins of those ten bits.
template <int LEVEL>
__global__ __launch_bounds__(256) void topk_hist_kernel(const float* __restrict__ w, const float* __restrict__ anchor,
                                                         const float* residual, float* vbuf,  // (may be one buffer)
                                                         uint32_t* __restrict__ hist, const uint32_t* __restrict__ state,
                                                         long long n4) {
#pragma clang fp contract(off)
  constexpr int BINS = LEVEL == 0 ? TK_H0 : TK_H1;
  __shared__ uint32_t h[BINS];
  const int lane = threadIdx.x & 63;
  for (int i = threadIdx.x; i < BINS; i += 256) h[i] = 0u;
  const uint32_t prefix = LEVEL == 0 ? 0u : state[ST_PREFIX];
  __syncthreads();
  for (long long base = blockIdx.x * 256ll; base < n4; base += (long long)gridDim.x * 256) {
    const long long f = base + threadIdx.x;
    const bool in = f < n4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (in) {
      if (LEVEL == 0) {
        const float4 x = reinterpret_cast<const float4*>(w)[f];
        const float4 a = reinterpret_cast<const float4*>(anchor)[f];
        v = make_float4(x.x - a.x, x.y - a.y, x.z - a.z, x.w - a.w);
        if (residual) {
          const float4 e = reinterpret_cast<const float4*>(residual)[f];
          v = make_float4(v.x + e.x, v.y + e.y, v.z + e.z, v.w + e.w);
        }
        reinterpret_cast<float4*>(vbuf)[f] = v;
      } else {
        v = reinterpret_cast<const float4*>(vbuf)[f];
      }
    }
    const uint32_t key[4] = {__float_as_uint(v.x) & 0x7fffffffu, __float_as_uint(v.y) & 0x7fffffffu,
                             __float_as_uint(v.z) & 0x7fffffffu, __float_as_uint(v.w) & 0x7fffffffu};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (LEVEL == 0) hist_add(h, key[c] >> 20, in, lane);
      if (LEVEL == 1) hist_add(h, (key[c] >> 10) & 1023u, in && (key[c] >> 20) == prefix, lane);
      if (LEVEL == 2) hist_add(h, key[c] & 1023u, in && (key[c] >> 10) == prefix, lane);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < BINS; i += 256) {
    const uint32_t c = h[i];
    if (c) atomicAdd(&hist[i], c);
  }
}

// One block.  Thread t owns the PER bins below BINS - t * PER, so thread 0 owns the top ones (at
// level 0 exactly the eight bins of the bad keys).  The bin that holds the rank-th largest key, and
// the rank that remains inside it.
template <int LEVEL>
__global__ __launch_bounds__(256) void topk_select_kernel(const uint32_t* __restrict__ hist, uint32_t* __restrict__ state,
                                                           uint32_t k, uint32_t n) {
  constexpr int BINS = LEVEL == 0 ? TK_H0 : TK_H1;
  constexpr int PER = BINS / 256;
  __shared__ uint32_t wtot[4];
  __shared__ uint32_t sh_bad;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int base = BINS - (t + 1) * PER;
  uint32_t c[PER], sum = 0u;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    c[j] = hist[base + j];
    sum += c[j];
  }
  uint32_t bad = 0u, keff, rank, prefix = 0u;
  if (LEVEL == 0) {
    if (t == 0) {
      sh_bad = sum;
#pragma unroll
      for (int j = 0; j < PER; ++j) c[j] = 0u;
      sum = 0u;
    }
    __syncthreads();
    bad = sh_bad;
    const uint32_t cand = n - bad;
    keff = k < cand ? k : cand;
    rank = keff;
  } else {
    keff = state[ST_KEFF];
    rank = state[ST_RANK];
    prefix = state[ST_PREFIX];
  }
  const uint32_t incl = tk_wave_scan_u32(sum, lane);
  if (lane == 63) wtot[wave] = incl;
  __syncthreads();  // (also: every thread has read the state before thread t writes it)
  uint32_t before = incl - sum;
  for (int w2 = 0; w2 < wave; ++w2) before += wtot[w2];
  if (keff == 0u) {  // nothing to send: no key matches the prefix, none exceeds or equals T
    if (t == 0) {
      state[ST_PREFIX] = TK_NONE;
      state[ST_RANK] = 0u;
      if (LEVEL == 0) {
        state[ST_BAD] = bad;
        state[ST_KEFF] = 0u;
      }
      if (LEVEL == 2) {
        state[ST_T] = TK_NONE;
        state[ST_BUDGET] = 0u;
      }
    }
    return;
  }
  if (before < rank && rank <= before + sum) {  // exactly one thread: 1 <= rank <= the total
    uint32_t acc = before;
    int bin = base;
    uint32_t left = 1u;
#pragma unroll
    for (int j = PER - 1; j >= 0; --j) {
      if (acc < rank && rank <= acc + c[j]) {
        bin = base + j;
        left = rank - acc;
      }
      acc += c[j];
    }
    const uint32_t np = LEVEL == 0 ? (uint32_t)bin : ((prefix << 10) | (uint32_t)bin);
    state[ST_PREFIX] = np;
    state[ST_RANK] = left;
    if (LEVEL == 0) {
      state[ST_BAD] = bad;
      state[ST_KEFF] = keff;
    }
    if (LEVEL == 2) {
      state[ST_T] = np;
      state[ST_BUDGET] = left;
    }
  }
}

// The packed counts of one float4 -- bits 0..15: keys > T (bad keys excluded), bits 16..31: keys == T
// -- and per component c the flags themselves in `bits`: bit c (> T), bit 4 + c (== T).
DEV uint32_t tk_flags(const float4& v, uint32_t T, bool in, uint32_t& bits) {
  const uint32_t key[4] = {__float_as_uint(v.x) & 0x7fffffffu, __float_as_uint(v.y) & 0x7fffffffu,
                           __float_as_uint(v.z) & 0x7fffffffu, __float_as_uint(v.w) & 0x7fffffffu};
  uint32_t p = 0u;
  bits = 0u;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const uint32_t g = (in && key[c] > T && key[c] < TK_BAD) ? 1u : 0u;
    const uint32_t q = (in && key[c] == T) ? 1u : 0u;
    p += g + (q << 16);
    bits |= (g << c) | (q << (4 + c));
  }
  return p;
}

__global__ __launch_bounds__(256) void topk_count_kernel(const float* __restrict__ vbuf, const uint32_t* __restrict__ state,
                                                          uint32_t* __restrict__ cnt, long long n, int chunks) {
  __shared__ uint32_t wsum[2][4];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const uint32_t T = state[ST_T];
  int par = 0;
  for (int b = blockIdx.x; b < chunks; b += gridDim.x, par ^= 1) {
    const long long e0 = (long long)b * TK_CHUNK;
    const int len = (int)std::min<long long>(TK_CHUNK, n - e0);
    uint32_t p = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int f = j * 256 + t;
      const bool in = f * 4 < len;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (in) v = reinterpret_cast<const float4*>(vbuf + e0)[f];
      uint32_t bits;
      p += tk_flags(v, T, in, bits);
    }
    p = tk_wave_sum_u32(p);  // <= 4096 in each half: no carry between them
    if (lane == 0) wsum[par][wave] = p;
    __syncthreads();
    if (t == 0) {
      const uint32_t s = wsum[par][0] + wsum[par][1] + wsum[par][2] + wsum[par][3];
      cnt[2ll * b] = s & 0xffffu;
      cnt[2ll * b + 1] = s >> 16;
    }
  }
}

// One block: offs[b] = exclusive scans of cnt over the chunks; payload[b] = entries sent in chunks < b
// = (keys > T before) + min(keys == T before, budget); payload[chunks] = k_eff.
__global__ __launch_bounds__(256) void topk_scan_kernel(const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ state,
                                                         uint32_t* __restrict__ offs, int32_t* __restrict__ payload,
                                                         int chunks) {
  __shared__ uint32_t wtot[2][4];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const uint32_t budget = state[ST_BUDGET];
  const int seg = (chunks + 255) / 256;
  const int lo = std::min(chunks, t * seg), hi = std::min(chunks, lo + seg);
  uint32_t sg = 0u, sq = 0u;
  for (int b = lo; b < hi; ++b) {
    sg += cnt[2ll * b];
    sq += cnt[2ll * b + 1];
  }
  const uint32_t ig = tk_wave_scan_u32(sg, lane), iq = tk_wave_scan_u32(sq, lane);
  if (lane == 63) {
    wtot[0][wave] = ig;
    wtot[1][wave] = iq;
  }
  __syncthreads();
  uint32_t g = ig - sg, q = iq - sq;
  for (int w2 = 0; w2 < wave; ++w2) {
    g += wtot[0][w2];
    q += wtot[1][w2];
  }
  for (int b = lo; b < hi; ++b) {
    offs[2ll * b] = g;
    offs[2ll * b + 1] = q;
    payload[b] = (int32_t)(g + (q < budget ? q : budget));
    g += cnt[2ll * b];
    q += cnt[2ll * b + 1];
  }
  if (t == 0) payload[chunks] = (int32_t)state[ST_KEFF];
}

__global__ __launch_bounds__(256) void topk_emit_kernel(const float* vbuf, float* residual,  // (may be one buffer)
                                                         const uint32_t* __restrict__ state, const uint32_t* __restrict__ offs,
                                                         int32_t* __restrict__ payload, double* __restrict__ partial,
                                                         uint32_t k, long long n, int chunks) {
#pragma clang fp contract(off)
  __shared__ uint32_t tot[2][16];  // [parity][sweep * 4 + wave]
  __shared__ double red[2][4];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const uint32_t T = state[ST_T], budget = state[ST_BUDGET], keff = state[ST_KEFF];
  uint32_t* vals = reinterpret_cast<uint32_t*>(payload) + chunks + 1;
  uint16_t* idx = reinterpret_cast<uint16_t*>(payload + chunks + 1 + (long long)k);
  double sum_v = 0.0, sum_e = 0.0;
  int par = 0;
  for (int b = blockIdx.x; b < chunks; b += gridDim.x, par ^= 1) {
    const long long e0 = (long long)b * TK_CHUNK;
    const int len = (int)std::min<long long>(TK_CHUNK, n - e0);
    const uint32_t goff = offs[2ll * b], qoff = offs[2ll * b + 1];
    const uint32_t rem = budget > qoff ? budget - qoff : 0u;  // keys == T this chunk may still send
    const uint32_t out0 = goff + (qoff < budget ? qoff : budget);
    float4 v[4];
    uint32_t p[4], incl[4], bits[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int f = j * 256 + t;
      const bool in = f * 4 < len;
      v[j] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (in) v[j] = reinterpret_cast<const float4*>(vbuf + e0)[f];
      p[j] = tk_flags(v[j], T, in, bits[j]);
      asm volatile("" : "+v"(bits[j]));  // (the 32 flags stay eight bits of a VGPR, not 32 wave predicates)
      incl[j] = tk_wave_scan_u32(p[j], lane);
      if (lane == 63) tot[par][j * 4 + wave] = incl[j];
    }
    __syncthreads();
    uint32_t run = 0u;  // the packed counts of every (sweep, wave) before this one, in index order
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      uint32_t mine = run;
#pragma unroll
      for (int w2 = 0; w2 < 4; ++w2) {
        const uint32_t s = tot[par][j * 4 + w2];
        mine += s & tk_lt_mask(w2, wave);
        run += s;
      }
      const uint32_t before = mine + incl[j] - p[j];
      uint32_t gb = before & 0xffffu, qb = before >> 16;
      const int f = j * 256 + t;
      const bool in = f * 4 < len;
      const float x[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
      float e[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const bool isbad = (__float_as_uint(x[c]) & 0x7fffffffu) >= TK_BAD;
        const bool g = (bits[j] >> c) & 1u, q = (bits[j] >> (4 + c)) & 1u;
        const bool send = g || (q && qb < rem);
        const uint32_t slot = out0 + gb + (qb < rem ? qb : rem);
        if (send && slot < keff) {
          vals[slot] = __float_as_uint(x[c]);
          idx[slot] = (uint16_t)(f * 4 + c);
        }
        gb += g ? 1u : 0u;
        qb += q ? 1u : 0u;
        e[c] = (send || isbad) ? 0.f : x[c];
        if (in && !isbad) {
          const double dv = (double)x[c], de = (double)e[c];
          sum_v = sum_v + dv * dv;
          sum_e = sum_e + de * de;
        }
      }
      if (residual && in) reinterpret_cast<float4*>(residual + e0)[f] = make_float4(e[0], e[1], e[2], e[3]);
    }
  }
  // entries k_eff .. k of the values and every index half from k_eff on: 0
  const long long halves = 2ll * ((k + 1ll) / 2);
  for (long long j = keff + blockIdx.x * 256ll + t; j < halves; j += (long long)gridDim.x * 256) {
    if (j < (long long)k) vals[j] = 0u;
    idx[j] = 0;
  }
  const double t0 = tk_wave_sum_f64(sum_v), t1 = tk_wave_sum_f64(sum_e);
  if (lane == 0) {
    red[0][wave] = t0;
    red[1][wave] = t1;
  }
  __syncthreads();
  if (t < 2) partial[2ll * blockIdx.x + t] = ((red[t][0] + red[t][1]) + red[t][2]) + red[t][3];
}

__global__ __launch_bounds__(256) void topk_finalize_kernel(const double* __restrict__ partial, int grid,
                                                             const uint32_t* __restrict__ state, double* __restrict__ stats) {
#pragma clang fp contract(off)
  double acc[2] = {0.0, 0.0};
  for (int i = threadIdx.x; i < grid; i += 256) {
    acc[0] = acc[0] + partial[2ll * i + 0];
    acc[1] = acc[1] + partial[2ll * i + 1];
  }
  __shared__ double red[2][4];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const double t0 = tk_wave_sum_f64(acc[0]), t1 = tk_wave_sum_f64(acc[1]);
  if (lane == 0) {
    red[0][wave] = t0;
    red[1][wave] = t1;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const double Sv = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
  const double Se = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
  const uint32_t keff = state[ST_KEFF];
  stats[0] = (double)(float)sqrt(Sv);
  stats[1] = (double)(float)sqrt(Se);
  stats[2] = (double)state[ST_BAD];
  stats[3] = (double)keff;
  stats[4] = keff ? (double)__uint_as_float(state[ST_T]) : 0.0;
  stats[5] = 0.0;
  stats[6] = 0.0;
  stats[7] = 0.0;
}

struct TopkDecodeArgs {
  const int32_t* src[TK_MAX_M];
  const float* anchor;
  float* out;
  bf16_t* shadow;  // nullable
  long long n;
  int chunks;
  int k;
  float inv;
};

template <int M>
__global__ __launch_bounds__(256) void topk_decode_mean_kernel(TopkDecodeArgs a) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) float acc[TK_CHUNK];
  const int t = threadIdx.x;
  for (int b = blockIdx.x; b < a.chunks; b += gridDim.x) {
    const long long e0 = (long long)b * TK_CHUNK;
    const int len = (int)std::min<long long>(TK_CHUNK, a.n - e0);
#pragma unroll
    for (int j = 0; j < 4; ++j) reinterpret_cast<float4*>(acc)[j * 256 + t] = make_float4(0.f, 0.f, 0.f, 0.f);
    __syncthreads();
#pragma unroll 1
    for (int c = 0; c < M; ++c) {
      const int32_t* __restrict__ src = a.src[c];
      const int lo = std::min(std::max(src[b], 0), a.k);
      const int hi = std::min(std::max(src[b + 1], lo), a.k);
      const uint32_t* vals = reinterpret_cast<const uint32_t*>(src) + a.chunks + 1;
      const uint32_t* idw = vals + a.k;
      for (int j = lo + t; j < hi; j += 256) {
        const uint32_t w = idw[j >> 1];
        const int li = (int)((j & 1) ? (w >> 16) : (w & 0xffffu));
        if (li < len) acc[li] = acc[li] + __uint_as_float(vals[j]);
      }
      __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int f = j * 256 + t;
      if (f * 4 < len) {
        const float4 s = reinterpret_cast<const float4*>(acc)[f];
        const float4 x = reinterpret_cast<const float4*>(a.anchor + e0)[f];
        const float m0 = s.x * a.inv, m1 = s.y * a.inv, m2 = s.z * a.inv, m3 = s.w * a.inv;
        const float4 o = make_float4(x.x + m0, x.y + m1, x.z + m2, x.w + m3);
        reinterpret_cast<float4*>(a.out + e0)[f] = o;
        if (a.shadow) reinterpret_cast<uint2*>(a.shadow + e0)[f] = make_uint2(pack_bf2(o.x, o.y), pack_bf2(o.z, o.w));
      }
    }
    __syncthreads();  // the accumulator is cleared again only after every thread has read it
  }
}

bool tk_overlap(const void* a, long long ab, const void* b, long long bb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + (uintptr_t)bb && b0 < a0 + (uintptr_t)ab;
}

template <int M>
bool tk_decode_launch(const TopkDecodeArgs& a, int grid, hipStream_t st) {
  hipLaunchKernelGGL((topk_decode_mean_kernel<M>), dim3(grid), dim3(256), 0, st, a);
  return true;
}

template <int... Ms>  // Ms = M - 1
bool tk_decode_m(int M, const TopkDecodeArgs& a, int grid, hipStream_t st, std::integer_sequence<int, Ms...>) {
  return ((M == Ms + 1 ? tk_decode_launch<Ms + 1>(a, grid, st) : false) || ...);
}

// every element index, count and payload word offset fits 31 bits
bool tk_n_ok(long long n) { return n > 0 && n % 64 == 0 && n <= 0x7fffffc0ll; }

}  // namespace

extern "C" {

// Blocks of the chunk-owning launches of fd_topk_encode / fd_topk_decode_mean over n floats.
int fd_topk_grid(long long n) { return tk_n_ok(n) ? tk_grid_for(n) : 0; }

// int32 words of the payload of n floats with k entries: ceil(n / 4096) + 1 offsets, k values,
// ceil(k / 2) words of uint16 local indices; 0 for an (n, k) that has no payload.
long long fd_topk_words(long long n, long long k) {
  if (!tk_n_ok(n) || k < 1 || k > n / 2) return 0;
  return tk_chunks(n) + 1 + k + (k + 1) / 2;
}

// Bytes of fd_topk_encode's `work` for n floats (16-byte aligned): v, the histograms and select
// state, the per-chunk counts and their scans, two doubles per block.
long long fd_topk_work_bytes(long long n) { return tk_n_ok(n) ? tk_work_bytes(n) : 0; }

// payload = the k largest-magnitude entries of (w - anchor) + residual over n floats (layout above),
// residual (nullable) = what was not sent, in place; stats[8] (doubles) = {|v|, |e'|, bad elements,
// sent, threshold, 0, 0, 0}.  n % 64 == 0, 1 <= k <= n / 2; no two buffers overlap.
int fd_topk_encode(const float* w, const float* anchor, float* residual, int32_t* payload, void* work, double* stats,
                   long long k, long long n, hipStream_t st) {
  if (!tk_n_ok(n)) return 1;
  if (!w || !anchor || !payload || !work || !stats) return 2;
  if (k < 1 || k > n / 2) return 3;
  if (((uintptr_t)work & 15u) != 0) return 4;
  const long long words = fd_topk_words(n, k), wbytes = tk_work_bytes(n);
  const void* bufs[6] = {w, anchor, residual, payload, work, stats};
  const long long bytes[6] = {n * 4, n * 4, n * 4, words * 4, wbytes, 64};
  for (int i = 0; i < 6; ++i)
    for (int j = i + 1; j < 6; ++j)
      if (bufs[i] && bufs[j] && tk_overlap(bufs[i], bytes[i], bufs[j], bytes[j])) return 5;
  const TopkWork wk = tk_carve(work, n);
  float* vbuf = residual ? residual : wk.v;
  const int chunks = (int)tk_chunks(n), grid = tk_grid_for(n);
  const long long n4 = n / 4;
  const dim3 g(grid), one(1), b(256);
  if (hipMemsetAsync(wk.hist, 0, (TK_H0 + TK_H1 + TK_H2 + TK_STATE) * 4ll, st) != hipSuccess) return 9;
  hipLaunchKernelGGL((topk_hist_kernel<0>), g, b, 0, st, w, anchor, (const float*)residual, vbuf, wk.hist,
                     (const uint32_t*)wk.state, n4);
  hipLaunchKernelGGL((topk_select_kernel<0>), one, b, 0, st, (const uint32_t*)wk.hist, wk.state, (uint32_t)k, (uint32_t)n);
  hipLaunchKernelGGL((topk_hist_kernel<1>), g, b, 0, st, w, anchor, (const float*)nullptr, vbuf, wk.hist + TK_H0,
                     (const uint32_t*)wk.state, n4);
  hipLaunchKernelGGL((topk_select_kernel<1>), one, b, 0, st, (const uint32_t*)(wk.hist + TK_H0), wk.state, (uint32_t)k,
                     (uint32_t)n);
  hipLaunchKernelGGL((topk_hist_kernel<2>), g, b, 0, st, w, anchor, (const float*)nullptr, vbuf, wk.hist + TK_H0 + TK_H1,
                     (const uint32_t*)wk.state, n4);
  hipLaunchKernelGGL((topk_select_kernel<2>), one, b, 0, st, (const uint32_t*)(wk.hist + TK_H0 + TK_H1), wk.state,
                     (uint32_t)k, (uint32_t)n);
  hipLaunchKernelGGL(topk_count_kernel, g, b, 0, st, (const float*)vbuf, (const uint32_t*)wk.state, wk.cnt, n, chunks);
  hipLaunchKernelGGL(topk_scan_kernel, one, b, 0, st, (const uint32_t*)wk.cnt, (const uint32_t*)wk.state, wk.offs, payload,
                     chunks);
  hipLaunchKernelGGL(topk_emit_kernel, g, b, 0, st, (const float*)vbuf, residual, (const uint32_t*)wk.state,
                     (const uint32_t*)wk.offs, payload, wk.partial, (uint32_t)k, n, chunks);
  hipLaunchKernelGGL(topk_finalize_kernel, one, b, 0, st, (const double*)wk.partial, grid, (const uint32_t*)wk.state, stats);
  return 0;
}

// out = anchor + mean of the M sparse payloads (in the given order) over n floats, shadow (nullable)
// = bf16(out).  1 <= M <= 16, n % 64 == 0, 1 <= k <= n / 2; out and shadow overlap no input.
int fd_topk_decode_mean(const int32_t* const* src, int M, const float* anchor, float* out, void* shadow, long long k,
                        long long n, hipStream_t st) {
  if (!tk_n_ok(n)) return 1;
  if (M < 1 || M > TK_MAX_M) return 2;
  if (k < 1 || k > n / 2) return 3;
  if (!src || !anchor || !out) return 4;
  const long long words = fd_topk_words(n, k);
  if (tk_overlap(out, n * 4, anchor, n * 4)) return 5;
  if (shadow && (tk_overlap(shadow, n * 2, anchor, n * 4) || tk_overlap(shadow, n * 2, out, n * 4))) return 5;
  TopkDecodeArgs a{};
  for (int s = 0; s < M; ++s) {
    if (!src[s]) return 4;
    if (tk_overlap(src[s], words * 4, out, n * 4) || (shadow && tk_overlap(src[s], words * 4, shadow, n * 2))) return 5;
    a.src[s] = src[s];
  }
  a.anchor = anchor;
  a.out = out;
  a.shadow = (bf16_t*)shadow;
  a.n = n;
  a.chunks = (int)tk_chunks(n);
  a.k = (int)k;
  a.inv = (float)(1.0 / (double)M);
  return tk_decode_m(M, a, tk_grid_for(n), st, std::make_integer_sequence<int, TK_MAX_M>{}) ? 0 : 2;
}

}  // extern "C"
