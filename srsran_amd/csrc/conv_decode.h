// srsran_amd/csrc/conv_decode.h -- one wave decodes one block of the LTE tail-biting convolutional code: rate
// dematching in LDS (rm_conv.c:98-148), u16 quantisation (viterbi.c:548-571), a 64-state tail-biting Viterbi decoder
// with one lane per trellis state (viterbi37_avx2_16bit.c semantics: wrapping u16 metrics, modular compare),
// chainback and CRC16.  Shared by the PDCCH blind search (pdcch_kernels.hip) and the PBCH decoder (pbch_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "pdcch_internal.h"

namespace mi355 {

namespace {

constexpr float    RX_NULL = 10000.0f;
#ifndef BLIND_DIAG
#define BLIND_DIAG 0 // (timing diagnostics: 1 stop after the gate, 2 after the branch-metric table, 3 after the Viterbi)
#endif
constexpr uint32_t MAXSYM  = 3 * PDCCH_MAX_F; // 432
// 30-step decision blocks the traceback reads: steps F + 6 .. 3F + 5
constexpr uint32_t tb_blocks()
{
  uint32_t m = 0;
  for (uint32_t F = 17; F <= PDCCH_MAX_F; F++) m = (3 * F + 5) / 30 - (F + 6) / 30 + 1 > m ? (3 * F + 5) / 30 - (F + 6) / 30 + 1 : m;
  return m;
}
constexpr uint32_t TB_BLOCKS = tb_blocks(); // 11
#ifndef VIT_ROTATE
#define VIT_ROTATE 1 // 1: rotating state layout with DPP / permlane partner exchange; 0: ds_bpermute gathers
#endif

// x^(d + 16) mod (x^16 + x^12 + x^5 + 1) for d < 128: the CRC16 contribution of a payload bit d places from the end
struct Crc16Pow {
  uint16_t v[128];
  constexpr Crc16Pow() : v()
  {
    uint32_t r = 0x1021u; // x^16 mod P
    for (int d = 0; d < 128; d++) {
      v[d] = (uint16_t)r;
      r    = (r << 1) ^ ((r & 0x8000u) ? 0x1021u : 0u);
      r &= 0xFFFFu;
    }
  }
};
__constant__ Crc16Pow c_crc16_pow_t = Crc16Pow();
#define c_crc16_pow (c_crc16_pow_t.v)

__constant__ uint8_t c_perm[32]     = {1, 17, 9, 25, 5, 21, 13, 29, 3, 19, 11, 27, 7, 23, 15, 31,
                                   0, 16, 8, 24, 4, 20, 12, 28, 2, 18, 10, 26, 6, 22, 14, 30};
__constant__ uint8_t c_perm_inv[32] = {16, 0, 24, 8, 20, 4, 28, 12, 18, 2, 26, 10, 22, 6, 30, 14,
                                       17, 1, 25, 9, 21, 5, 29, 13, 19, 3, 27, 11, 23, 7, 31, 15};

// 5,600 B per wave (29 waves per CU by LDS): every array shares storage with one that is dead by the time it is
// written -- bm and the decoded bits with the rate-dematching buffers, the decision strings with the quantised
// symbols (the Viterbi reads the branch-metric table only) -- and only the decision blocks the traceback reads are
// kept
struct WaveLds {
  union {
    struct {
      float    tmp[3 * 32 * 5];  // rate-dematching circular buffer (3 K_pi, K_pi <= 160)
      uint16_t rank_pos[MAXSYM]; // position of the r-th non-dummy bit in the circular buffer
    };
    struct {
      uint16_t bm[PDCCH_MAX_F * 8]; // branch metric per (t mod F, encoder output pattern), once the above are dead
      uint8_t  bits[PDCCH_MAX_F];   // decoded bits (middle repetition), written by the traceback
    };
  };
  union {
    uint16_t q[MAXSYM];          // quantised soft symbols, dead once bm is built
    uint32_t tdec[TB_BLOCKS][64]; // Viterbi decisions, lane-major bit strings of 30 steps (blocks tb0 .. tb1)
  };
};

__device__ __forceinline__ double wave_sum(double v)
{
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v)
{
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ uint32_t wave_min(uint32_t v)
{
  for (int o = 32; o > 0; o >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, o, 64));
  return v;
}

// lane k of (lo, hi) := the two halves of w (w and k wave-uniform; the lane select goes through M0, one SGPR
// operand per VALU instruction).  M0 is reserved, so the compiler keeps no value in it across code that does not
// set it up right before use (nothing else in this file does); clang warns that it does not track the clobber.
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
__device__ __forceinline__ void writelane2(uint32_t& lo, uint32_t& hi, uint64_t w, uint32_t k)
{
  asm volatile("s_mov_b32 m0, %4\n\tv_writelane_b32 %0, %2, m0\n\tv_writelane_b32 %1, %3, m0"
               : "+v"(lo), "+v"(hi)
               : "s"((uint32_t)w), "s"((uint32_t)(w >> 32)), "s"(k)
               : "m0");
}
__device__ __forceinline__ void writelane1(uint32_t& v, uint32_t x, uint32_t k)
{
  asm volatile("s_mov_b32 m0, %2\n\tv_writelane_b32 %0, %1, m0" : "+v"(v) : "s"(x), "s"(k) : "m0");
}
#pragma clang diagnostic pop

__device__ __forceinline__ uint32_t par(uint32_t x) { return __builtin_popcount(x) & 1u; }
__device__ __forceinline__ uint32_t rotl6(uint32_t x, uint32_t r) { return ((x << r) | (x >> (6 - r))) & 63u; }
__device__ __forceinline__ uint32_t rotr6(uint32_t x, uint32_t r) { return ((x >> r) | (x << (6 - r))) & 63u; }

// One trellis step of the 64-state Viterbi in the rotating layout.  At phase K lane l holds state rotl6(l, K), so the
// predecessors j and j + 32 of a successor pair (2j, 2j + 1) sit in the lanes l and l ^ (32 >> K), and the pair's
// successors land in the same two lanes at phase K + 1 (rotr6(2j, K + 1) = rotr6(j, K)): every step exchanges with
// one fixed partner -- a permlane32 / permlane16 swap, DPP row shifts under a bank mask, DPP quad permutes -- in place
// of two ds_bpermute gathers through LDS.  X / Y: the metric of the pair's low / high predecessor, in both lanes.
// Returns the decision (survivor from j + 32); xa: this lane's branch metric, complemented for the odd successor.
template <int K> __device__ __forceinline__ bool vit_step(uint32_t& met, uint32_t xa)
{
  uint32_t X, Y;
  if constexpr (!VIT_ROTATE) { // identity layout: state s takes predecessors s >> 1 and (s >> 1) + 32
    const int j = (int)(__lane_id() >> 1);
    X           = (uint32_t)__shfl((int)met, j, 64);
    Y           = (uint32_t)__shfl((int)met, j + 32, 64);
  } else if constexpr (K == 0) {
    const auto r = __builtin_amdgcn_permlane32_swap(met, met, false, false);
    X = r[0], Y = r[1];
  } else if constexpr (K == 1) {
    const auto r = __builtin_amdgcn_permlane16_swap(met, met, false, false);
    X = r[0], Y = r[1];
  } else if constexpr (K == 2) { // partner 8 apart: row_shr:8 into banks 2-3, row_shl:8 into banks 0-1
    X = (uint32_t)__builtin_amdgcn_update_dpp((int)met, (int)met, 0x118, 0xF, 0xC, false);
    Y = (uint32_t)__builtin_amdgcn_update_dpp((int)met, (int)met, 0x108, 0xF, 0x3, false);
  } else if constexpr (K == 3) { // 4 apart: row_shr:4 into banks 1 and 3, row_shl:4 into banks 0 and 2
    X = (uint32_t)__builtin_amdgcn_update_dpp((int)met, (int)met, 0x114, 0xF, 0xA, false);
    Y = (uint32_t)__builtin_amdgcn_update_dpp((int)met, (int)met, 0x104, 0xF, 0x5, false);
  } else if constexpr (K == 4) { // 2 apart: quad_perm [0,1,0,1] / [2,3,2,3]
    X = (uint32_t)__builtin_amdgcn_mov_dpp((int)met, 0x44, 0xF, 0xF, true);
    Y = (uint32_t)__builtin_amdgcn_mov_dpp((int)met, 0xEE, 0xF, 0xF, true);
  } else { // 1 apart: quad_perm [0,0,2,2] / [1,1,3,3]
    X = (uint32_t)__builtin_amdgcn_mov_dpp((int)met, 0xA0, 0xF, 0xF, true);
    Y = (uint32_t)__builtin_amdgcn_mov_dpp((int)met, 0xF5, 0xF, 0xF, true);
  }
  const uint32_t x = X + xa, y = (xa ^ 8191u) + Y; // only the low 16 bits matter (wrapping u16 metrics)
  const bool     d = (int16_t)(uint16_t)(x - y) > 0;
  met              = d ? y : x;
  return d;
}

// Decode one candidate that passed the gate: rate dematching (rm_conv.c:98-148), the AVX2 decoder's quantisation, a
// 64-state tail-biting Viterbi over three repetitions and its chainback, CRC16 remainder.  Lane 0 writes out (status
// 2); returns the CRC remainder (wave-uniform) and w0 = payload bits 0..31, MSB first.
// SCALED (the PBCH, pbch.c:420): the dematched values are multiplied by scale before the quantisation.
template <bool SCALED = false>
__device__ __forceinline__ uint32_t decode_cand(WaveLds& S, const float* llr, uint32_t E, uint32_t nbits, uint32_t L,
                                                uint32_t ncce, DciCand* out, uint32_t& w0, float scale = 1.f)
{
  const uint32_t lane = __lane_id();
  // rate dematching (rm_conv.c:98-148)
  const uint32_t F = nbits + 16, N = 3 * F;
  const uint32_t nrows = (F - 1) / 32 + 1, Kp = 32 * nrows, ndummy = Kp - F;
  const float    rcp_rows = 1.0f / (float)nrows;
  for (uint32_t j = lane; j < 3 * Kp; j += 64) S.tmp[j] = RX_NULL;
  uint32_t run = 0;
  for (uint32_t base = 0; base < 3 * Kp; base += 64) {
    // jj = j mod Kp and jj = qn * nrows + rn without integer division (j < 3 Kp + 64, jj < 160, nrows <= 5:
    // (jj + 0.5) / nrows sits at least 0.1 away from an integer, far beyond float rounding)
    const uint32_t j  = base + lane, jj = j >= 2 * Kp ? j - 2 * Kp : j >= Kp ? j - Kp : j;
    const uint32_t qn = (uint32_t)(((float)jj + 0.5f) * rcp_rows), rn = jj - qn * nrows;
    const bool     v  = j < 3 * Kp && rn * 32 + c_perm[qn & 31] >= ndummy;
    const uint64_t m = __ballot(v);
    if (v) S.rank_pos[run + __popcll(m & ((1ull << lane) - 1))] = (uint16_t)j;
    run += __popcll(m);
  }
  __builtin_amdgcn_wave_barrier();
  for (uint32_t r = lane; r < N; r += 64) {
    float v = RX_NULL;
    for (uint32_t i = r; i < E; i += N) {
      const float x = llr[i];
      if (v == RX_NULL)
        v = x;
      else if (x != RX_NULL)
        v += x;
    }
    S.tmp[S.rank_pos[r]] = v;
  }
  __builtin_amdgcn_wave_barrier();
  // bit selection back to (s0, s1, s2) triples, then |max| and u16 quantisation (FMA as the AVX2 build)
  float mx = 0.f, rmv[7];
  for (uint32_t u = 0, i = lane; u < 7; u++, i += 64) {
    rmv[u] = 0.f;
    if (i < N) {
      const uint32_t t = i / 3, st = i % 3, di = (t + ndummy) / 32, dj = (t + ndummy) % 32;
      const float    o = S.tmp[Kp * st + c_perm_inv[dj] * nrows + di];
      rmv[u]           = o != RX_NULL ? o : 0.f;
      if constexpr (SCALED) rmv[u] *= scale;
      mx               = fmaxf(mx, fabsf(rmv[u]));
    }
  }
  mx = fmaxf(wave_max(mx), 1e-9f);
  const float gain = 1000.0f / mx;
  for (uint32_t u = 0, i = lane; u < 7; u++, i += 64) {
    if (i < N) {
      int32_t q = (int32_t)__builtin_fmaf(gain, rmv[u], 32767.5f);
      q         = q < 0 ? 0 : q > 65535 ? 65535 : q;
      S.q[i]    = (uint16_t)q;
    }
  }
  __builtin_amdgcn_wave_barrier();
  // the branch metric of step t depends only on the symbol triple (t mod F) and the state's encoder output pattern
  // (8 of them): tabulate it once instead of recomputing it 3 times per trellis step in all 64 lanes
  for (uint32_t e = lane; e < 8 * F; e += 64) {
    const uint32_t o = 3 * (e >> 3), pt = e & 7u;
    const uint32_t c0 = (pt & 1u) ? 0xFFFFu : 0u, c1 = (pt & 2u) ? 0xFFFFu : 0u, c2 = (pt & 4u) ? 0xFFFFu : 0u;
    const uint32_t av = ((c0 ^ S.q[o]) + (c1 ^ S.q[o + 1]) + 1) >> 1;
    S.bm[e]           = (uint16_t)((((c2 ^ S.q[o + 2]) + av + 1) >> 1) >> 3);
  }
  __builtin_amdgcn_wave_barrier();
  if (BLIND_DIAG == 2) return ~0u;
  // 64-state Viterbi over 3F steps, one lane per state (vit_step), decisions kept as per-lane bit strings: step
  // 30 b + r's decision of lane l is bit 29 - r of tdec[b - tb0][l] (one v_addc per step, one 64-lane store per 30
  // steps; 30 is a multiple of the state layout's period).  Only the blocks the traceback reads are kept: steps
  // F + 6 .. 3F + 5 (decision of step n read at n + 6, as the AVX2 traceback), the ones past 3F - 1 zero
  const uint32_t Fs = __builtin_amdgcn_readfirstlane(F); // uniform: the step counters live in scalar registers
  const uint32_t tb0 = (Fs + 6) / 30, tb1 = (3 * Fs + 5) / 30;
  // per phase k: the branch-metric pattern of the lane's pair (encoder output of its low predecessor j doubled) and
  // whether the lane takes the odd successor (the complemented metric; 13-bit metrics: 8191 - m = m ^ 8191)
  uint32_t boff[6], flip[6];
#pragma unroll
  for (uint32_t k = 0; k < 6; k++) {
    const uint32_t j = (VIT_ROTATE ? rotl6(lane, k) : lane >> 1) & 31u;
    boff[k]          = par((2 * j) & 0x6Du) | par((2 * j) & 0x4Fu) << 1 | par((2 * j) & 0x57u) << 2;
    flip[k]          = (VIT_ROTATE ? (lane >> (5 - k)) & 1u : lane & 1u) ? 8191u : 0u;
  }
  uint32_t met = 0, o = 0;
  // branch metrics of the next six steps, read one group ahead so that no LDS latency sits on the metric chain
  uint32_t cur[6], nxt[6];
  const auto load6 = [&](uint32_t* xa) {
#pragma unroll
    for (int K = 0; K < 6; K++) {
      xa[K] = (uint32_t)S.bm[8 * o + boff[K]] ^ flip[K];
      o     = (o + 1 == Fs) ? 0 : o + 1;
    }
  };
  load6(cur);
  for (uint32_t tb = 0, b = 0; tb < 3 * Fs; tb += 30, b++) {
    const uint32_t te   = __builtin_amdgcn_readfirstlane(min(3 * Fs - tb, 30u));
    uint32_t       dreg = 0, k = 0;
#define VIT_STEP(K)                                                                                                   \
  do {                                                                                                               \
    const bool d = vit_step<K>(met, cur[K]);                                                                         \
    dreg         = dreg + dreg + (uint32_t)d;                                                                        \
    k++;                                                                                                             \
  } while (0)
    while (k + 6 <= te) {
      load6(nxt); // (past the last step these read valid, unused entries)
      VIT_STEP(0);
      VIT_STEP(1);
      VIT_STEP(2);
      VIT_STEP(3);
      VIT_STEP(4);
      VIT_STEP(5);
#pragma unroll
      for (int K = 0; K < 6; K++) cur[K] = nxt[K];
    }
    if (k < te) { // (the last block only: 3F need not be a multiple of 6)
      VIT_STEP(0);
      if (k < te) {
        VIT_STEP(1);
        if (k < te) {
          VIT_STEP(2);
          if (k < te) {
            VIT_STEP(3);
            if (k < te) VIT_STEP(4);
          }
        }
      }
    }
#undef VIT_STEP
    if (b >= tb0) S.tdec[b - tb0][lane] = dreg << (30 - te);
  }
  if (tb1 > (3 * Fs - 1) / 30) S.tdec[tb1 - tb0][lane] = 0;
  if (BLIND_DIAG == 3) {
    if (met == 12345678u) out->L = 9; // (keeps the Viterbi live)
    return ~0u;
  }
  met &= 0xFFFFu;
  // best end state: the last index of the smallest (unsigned) metric; after 3F steps lane l holds state
  // rotl6(l, 3F mod 6) in the rotating layout
  const uint32_t pe   = VIT_ROTATE ? (3 * Fs) % 6 : 0u;
  const uint32_t key  = wave_min((met << 6) | (63u - rotl6(lane, pe)));
  const uint32_t best = 63u - ((uint32_t)__builtin_amdgcn_readfirstlane((int)key) & 63u);
  __builtin_amdgcn_wave_barrier();
  // chainback from step 3F - 1 down to F, walking the survivor's LANE in a scalar register: the decision of step
  // n + 6 for it is one readlane of that block's bit strings.  Identity layout: state s -> (s >> 1) | kb << 5.
  // Rotating layout: the decision of step t sits in lane rotr6(s, (t + 1) mod 6) and one step back the predecessor's
  // lane is the same lane with bit (5 - t mod 6) mod 6 ... i.e. bit (6 - (t + 1) mod 6) mod 6 replaced by kb.
  // Decoded bits of the middle repetition (n < 2F) are gathered per block (acc: bit i = step t_lo + i) and stored
  // once per block.
  uint32_t ln = rotr6(best, pe);
  for (int b = (int)tb1; b >= (int)tb0; b--) {
    const uint32_t tr  = S.tdec[b - (int)tb0][lane];
    const int      t0  = 30 * b;
    const int      rhi = min(29, (int)(3 * Fs + 5) - t0), rlo = max(0, (int)(Fs + 6) - t0);
    uint32_t       acc = 0;
#define TB_STEP(R)                                                                                                    \
  do {                                                                                                               \
    const uint32_t kb = ((uint32_t)__builtin_amdgcn_readlane((int)tr, (int)ln) >> (29 - (R))) & 1u;                  \
    if (VIT_ROTATE) {                                                                                                \
      constexpr uint32_t q = (6u - ((R) + 1u) % 6u) % 6u;                                                            \
      ln                   = (ln & ~(1u << q)) | (kb << q);                                                          \
    } else {                                                                                                         \
      ln = (ln >> 1) | (kb << 5);                                                                                    \
    }                                                                                                                \
    acc = acc + acc + kb;                                                                                            \
  } while (0)
#define TB_STEP_IF(R)                                                                                                 \
  if ((R) <= rhi && (R) >= rlo) TB_STEP(R)
    if (rhi == 29 && rlo == 0) {
      TB_STEP(29); TB_STEP(28); TB_STEP(27); TB_STEP(26); TB_STEP(25); TB_STEP(24);
      TB_STEP(23); TB_STEP(22); TB_STEP(21); TB_STEP(20); TB_STEP(19); TB_STEP(18);
      TB_STEP(17); TB_STEP(16); TB_STEP(15); TB_STEP(14); TB_STEP(13); TB_STEP(12);
      TB_STEP(11); TB_STEP(10); TB_STEP(9); TB_STEP(8); TB_STEP(7); TB_STEP(6);
      TB_STEP(5); TB_STEP(4); TB_STEP(3); TB_STEP(2); TB_STEP(1); TB_STEP(0);
    } else {
      TB_STEP_IF(29); TB_STEP_IF(28); TB_STEP_IF(27); TB_STEP_IF(26); TB_STEP_IF(25); TB_STEP_IF(24);
      TB_STEP_IF(23); TB_STEP_IF(22); TB_STEP_IF(21); TB_STEP_IF(20); TB_STEP_IF(19); TB_STEP_IF(18);
      TB_STEP_IF(17); TB_STEP_IF(16); TB_STEP_IF(15); TB_STEP_IF(14); TB_STEP_IF(13); TB_STEP_IF(12);
      TB_STEP_IF(11); TB_STEP_IF(10); TB_STEP_IF(9); TB_STEP_IF(8); TB_STEP_IF(7); TB_STEP_IF(6);
      TB_STEP_IF(5); TB_STEP_IF(4); TB_STEP_IF(3); TB_STEP_IF(2); TB_STEP_IF(1); TB_STEP_IF(0);
    }
#undef TB_STEP_IF
#undef TB_STEP
    // step t = t0 + rlo + i decoded bit i of acc; it is bit n - F of the block for n = t - 6 in [F, 2F)
    const int n = t0 + rlo + (int)lane - 6;
    if ((int)lane <= rhi - rlo && n < 2 * (int)Fs) S.bits[n - (int)Fs] = (uint8_t)((acc >> lane) & 1u);
  }
  __builtin_amdgcn_wave_barrier();
  // CRC16 (crc.c, poly 0x1021, zero init: payload(x) * x^16 mod P) is linear in the payload bits: bit i contributes
  // x^(nbits - 1 - i + 16) mod P, so every lane takes its bits' terms and the wave xor-reduces; the payload words
  // (MSB first) and the received parity come from ballots of the decoded bits -- no serial per-bit loop on one lane
  uint32_t rem = 0;
  if (F > 128) { // the serial form: no LTE DCI is this long, but MI355_DCI_MAX_BITS admits payloads of 113..128 bits
    if (lane == 0) {
      uint32_t crc = 0, p = 0;
      for (uint32_t i = 0; i < nbits; i++) {
        const uint32_t fb = ((crc >> 15) ^ S.bits[i]) & 1u;
        crc               = (crc << 1) & 0xFFFFu;
        if (fb) crc ^= 0x1021u;
      }
      for (uint32_t i = 0; i < 16; i++) p = (p << 1) | S.bits[nbits + i];
      out->status = 2, out->crc_rem = p ^ crc, out->L = L, out->ncce = ncce;
      for (uint32_t q = 0; q < 4; q++) {
        uint32_t w = 0;
        for (uint32_t b = 0; b < 32; b++)
          if (32 * q + b < nbits) w |= (uint32_t)S.bits[32 * q + b] << (31 - b);
        out->bits[q] = w;
      }
      rem = p ^ crc, w0 = out->bits[0];
    }
    rem = (uint32_t)__builtin_amdgcn_readfirstlane((int)rem);
    w0  = (uint32_t)__builtin_amdgcn_readfirstlane((int)w0);
    return rem;
  }
  uint32_t       crc = 0;
  const uint32_t b0 = lane < F ? S.bits[lane] : 0u, b1 = lane + 64 < F ? S.bits[lane + 64] : 0u;
  if (lane < nbits && b0) crc ^= c_crc16_pow[nbits - 1 - lane];
  if (lane + 64 < nbits && b1) crc ^= c_crc16_pow[nbits - 1 - (lane + 64)];
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) crc ^= (uint32_t)__shfl_xor((int)crc, o, 64);
  const uint64_t m0 = __ballot(b0 != 0), m1 = __ballot(b1 != 0); // bit i of the decoded block: lane i of (m0, m1)
  if (lane == 0) {
    // the 16 parity bits follow the payload, MSB first: bits nbits .. nbits + 15 of the 128-bit (m1:m0)
    const uint32_t sh = nbits, p = (uint32_t)__builtin_bitreverse32(
                                       (uint32_t)(sh < 64 ? (m0 >> sh) | (sh ? m1 << (64 - sh) : 0ull) : m1 >> (sh - 64))) >>
                                   16;
    out->status  = 2;
    out->crc_rem = p ^ crc;
    out->L       = L;
    out->ncce    = ncce;
    const uint32_t w[4] = {(uint32_t)m0, (uint32_t)(m0 >> 32), (uint32_t)m1, (uint32_t)(m1 >> 32)};
#pragma unroll
    for (uint32_t q = 0; q < 4; q++) {
      const uint32_t n = nbits > 32 * q ? min(32u, nbits - 32 * q) : 0u; // payload bits in word q
      out->bits[q]     = n ? __builtin_bitreverse32(w[q]) & (0xFFFFFFFFu << (32 - n)) : 0u;
    }
    rem = p ^ crc;
  }
  w0 = __builtin_bitreverse32((uint32_t)m0); // payload bits 0 .. 31, MSB first (bits past nbits are not looked at)
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)rem);
}

} // namespace

} // namespace mi355
