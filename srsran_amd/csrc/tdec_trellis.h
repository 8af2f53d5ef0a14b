// srsran_amd/csrc/tdec_trellis.h
//
// The 8-state trellis of the LTE turbo code on packed int16 pairs (device code), shared by the window MAP kernel
// (tdec_kernels.hip), the generic decoder (tdec_gen.hip) and the latency kernel (tdec_win_lat.hip): every 32-bit
// register holds two int16 metrics (two windows, or two code blocks), so each operation is one v_pk_* instruction.
// SAT selects the window decoders' saturating arithmetic (turbodecoder_win.h, _mm256_adds_epi16) or the generic
// decoder's and the tail trellis' wrapping one (turbodecoder_gen.c).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tdec_internal.h"

namespace mi355 {

typedef short v2s __attribute__((ext_vector_type(2)));

__device__ __forceinline__ v2s U(uint32_t u) { return __builtin_bit_cast(v2s, u); }
__device__ __forceinline__ uint32_t W(v2s v) { return __builtin_bit_cast(uint32_t, v); }
__device__ __forceinline__ v2s sadd(v2s a, v2s b) { return __builtin_elementwise_add_sat(a, b); }
__device__ __forceinline__ v2s ssub(v2s a, v2s b) { return __builtin_elementwise_sub_sat(a, b); }
__device__ __forceinline__ v2s vmax(v2s a, v2s b) { return __builtin_elementwise_max(a, b); }
__device__ __forceinline__ v2s splat(short s) { return (v2s){s, s}; }

template <bool SAT>
__device__ __forceinline__ v2s add(v2s a, v2s b)
{
  if constexpr (SAT) {
    return sadd(a, b);
  } else {
    return a + b;
  }
}

template <bool SAT>
__device__ __forceinline__ v2s sub(v2s a, v2s b)
{
  if constexpr (SAT) {
    return ssub(a, b);
  } else {
    return a - b;
  }
}

// State numbering reg0<<2|reg1<<1|reg2, branch metric u*x + p*y (turbocoder.c:403-421).

// beta row n of a step from the row o after it (turbodecoder_win.h:640-676, turbodecoder_gen.c:58-112)
template <bool SAT>
__device__ __forceinline__ void beta_step(const v2s o[8], v2s x, v2s y, v2s n[8])
{
  v2s xy = add<SAT>(x, y);
  n[0]   = vmax(add<SAT>(o[4], xy), o[0]);
  n[1]   = vmax(o[4], add<SAT>(o[0], xy));
  n[2]   = vmax(add<SAT>(o[5], y), add<SAT>(o[1], x));
  n[3]   = vmax(add<SAT>(o[5], x), add<SAT>(o[1], y));
  n[4]   = vmax(add<SAT>(o[6], x), add<SAT>(o[2], y));
  n[5]   = vmax(add<SAT>(o[6], y), add<SAT>(o[2], x));
  n[6]   = vmax(o[7], add<SAT>(o[3], xy));
  n[7]   = vmax(add<SAT>(o[7], xy), o[3]);
}

// the two candidates (input bit 0 / 1) of every alpha state after a step from the states o entering it
// (turbodecoder_win.h:771-800): the next state is their max, the output LLR takes them one by one
template <bool SAT>
__device__ __forceinline__ void alpha_cands(const v2s o[8], v2s x, v2s y, v2s c0[8], v2s c1[8])
{
  v2s xy = add<SAT>(x, y);
  c0[0]  = o[0];
  c1[0]  = add<SAT>(o[1], xy);
  c0[1]  = add<SAT>(o[3], y);
  c1[1]  = add<SAT>(o[2], x);
  c0[2]  = add<SAT>(o[4], y);
  c1[2]  = add<SAT>(o[5], x);
  c0[3]  = o[7];
  c1[3]  = add<SAT>(o[6], xy);
  c0[4]  = o[1];
  c1[4]  = add<SAT>(o[0], xy);
  c0[5]  = add<SAT>(o[2], y);
  c1[5]  = add<SAT>(o[3], x);
  c0[6]  = add<SAT>(o[5], y);
  c1[6]  = add<SAT>(o[4], x);
  c0[7]  = o[6];
  c1[7]  = add<SAT>(o[7], xy);
}

template <bool SAT>
__device__ __forceinline__ void normalize(v2s s[8])
{
#pragma unroll
  for (int i = 1; i < 8; i++) s[i] = sub<SAT>(s[i], s[0]);
  s[0] = splat(0);
}

__device__ __forceinline__ void set_minf(v2s s[8])
{
#pragma unroll
  for (int i = 0; i < 8; i++) s[i] = splat(-TDEC_INF);
}

// (The window decoders' output LLR, a max tree over sat(beta row + candidate), is not here: taken from a shared
// function, the window MAP kernel's instantiations come out scheduled differently, so tdec_kernels.hip and
// tdec_win_lat.hip each keep theirs.)

} // namespace mi355
