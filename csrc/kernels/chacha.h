// The ChaCha block function of RFC 8439 section 2.3 (Bernstein, "ChaCha, a variant of Salsa20", 2008)
// with 8, 12 or 20 rounds: the pseudorandom generator of secagg.hip (pairwise masks of the secure
// aggregation).  parallel/secagg.py chacha_block mirrors it on the host bit for bit.
//
// Four consecutive lanes (an aligned quad) share one 16-word block: lane c of the quad owns column c
// of the 4 x 4 state -- a = x[c] (constant), b = x[4 + c] and cc = x[8 + c] (key), d = x[12 + c]
// (counter, nonce).  A column round is a quarter round inside the lane; for the diagonal round the
// b, cc and d rows move one, two and three lanes round the quad (DPP quad_perm, no LDS) and back.
// The lane leaves with the four words {x[c], x[4 + c], x[8 + c], x[12 + c]} of the block: they are
// the mask words of the lane's float4, so element e of a block (0 .. 15) takes RFC word
// 4 * (e % 4) + e / 4 -- the transposed order -- and loads and stores stay float4-wide and coalesced.
// All four lanes of a quad must be active together.
//
// A rotate is one v_alignbit_b32 (__builtin_rotateleft32).  U independent blocks (one per partner
// key) go through the rounds side by side to cover the add - xor - rotate dependency chain.
#pragma once
#include "common.h"

constexpr uint32_t CHACHA_C0 = 0x61707865u, CHACHA_C1 = 0x3320646eu, CHACHA_C2 = 0x79622d32u, CHACHA_C3 = 0x6b206574u;

// lane i of a quad reads lane (i + K) % 4 of it
template <int K>
DEV uint32_t chacha_quad_rot(uint32_t v) {
  static_assert(K >= 1 && K <= 3, "quad rotation");
  constexpr int ctrl = K == 1 ? 0x39 : K == 2 ? 0x4E : 0x93;  // quad_perm:[1,2,3,0] / [2,3,0,1] / [3,0,1,2]
  return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, ctrl, 0xf, 0xf, true);
}

#define CHACHA_QR(a, b, c, d)            \
  a += b;                                \
  d ^= a;                                \
  d = __builtin_rotateleft32(d, 16);     \
  c += d;                                \
  b ^= c;                                \
  b = __builtin_rotateleft32(b, 12);     \
  a += b;                                \
  d ^= a;                                \
  d = __builtin_rotateleft32(d, 8);      \
  c += d;                                \
  b ^= c;                                \
  b = __builtin_rotateleft32(b, 7);

// This lane's column of U blocks.  col = lane & 3; kb[u] = key_u[col], kc[u] = key_u[4 + col];
// d0 = {counter, nonce0, nonce1, nonce2}[col] (shared by the U blocks: one counter, one nonce, U keys).
// out[u] = {x[col], x[4 + col], x[8 + col], x[12 + col]} of block u.
template <int ROUNDS, int U>
DEV void chacha_columns(int col, const uint32_t (&kb)[U], const uint32_t (&kc)[U], uint32_t d0, uint4 (&out)[U]) {
  static_assert(ROUNDS == 8 || ROUNDS == 12 || ROUNDS == 20, "ChaCha8, ChaCha12 or ChaCha20");
  const uint32_t a0 = col == 0 ? CHACHA_C0 : col == 1 ? CHACHA_C1 : col == 2 ? CHACHA_C2 : CHACHA_C3;
  uint32_t a[U], b[U], c[U], d[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    a[u] = a0;
    b[u] = kb[u];
    c[u] = kc[u];
    d[u] = d0;
  }
#pragma unroll
  for (int r = 0; r < ROUNDS; r += 2) {
#pragma unroll
    for (int u = 0; u < U; ++u) { CHACHA_QR(a[u], b[u], c[u], d[u]) }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      b[u] = chacha_quad_rot<1>(b[u]);
      c[u] = chacha_quad_rot<2>(c[u]);
      d[u] = chacha_quad_rot<3>(d[u]);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) { CHACHA_QR(a[u], b[u], c[u], d[u]) }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      b[u] = chacha_quad_rot<3>(b[u]);
      c[u] = chacha_quad_rot<2>(c[u]);
      d[u] = chacha_quad_rot<1>(d[u]);
    }
  }
#pragma unroll
  for (int u = 0; u < U; ++u) out[u] = make_uint4(a[u] + a0, b[u] + kb[u], c[u] + kc[u], d[u] + d0);
}
