// srsran_amd/csrc/pdcch_kernels.hip -- downlink control channels on gfx950.
//
//   ctrl_llr      one workgroup per subframe: PCFICH (16 REs -> CFI by correlation with the three code words,
//                 pcfich.c:120-225), then the PDCCH REs of that CFI (REG map in HBM) equalised for transmit
//                 diversity / single port, QPSK-demapped and descrambled into float LLRs (pdcch.c:410-460).
//   pdcch_blind   one wave per (subframe, search-space candidate, DCI size): mean |LLR| gate, convolutional
//                 rate dematching in LDS (rm_conv.c:98-148), u16 quantisation (viterbi.c:548-571), a 64-state
//                 tail-biting Viterbi decoder with one lane per trellis state (cross-lane reads by ds_bpermute,
//                 decision words by ballot into LDS; viterbi37_avx2_16bit.c semantics: wrapping u16 metrics,
//                 modular compare), chainback and CRC16 -> the CRC remainder the host compares with the RNTI.
//   pdcch_compact one wave per subframe: the candidates whose remainder is the searched RNTI, in slot order (the
//                 only ones the host replay acts on) -> the small per-subframe record the host reads back.
//   conv_decode_debug  inspection (mi355_debug_conv_decode_batch): one wave per caller-given vector through gate_pass /
//                 decode_cand as pdcch_blind and pbch_decode call them, for parity tests at every block length.
//
// Integer / byte-level work throughout; nothing here is GEMM-shaped.  The equaliser evaluates the reference's
// formulas without FMA contraction (built with -ffp-contract=off) so it equals oracle/orc_pdcch.c bit for bit.
// The equalisers / demapper (ctrl_eq.h) and the candidate decoder (conv_decode.h) are shared with the PBCH kernels.
#include <hip/hip_runtime.h>

#include "conv_decode.h"
#include "ctrl_eq.h"
#include "pdcch_internal.h"

namespace mi355 {

namespace {

__device__ __forceinline__ uint32_t seq_bit(const uint32_t* s, uint32_t i) { return (s[i >> 5] >> (i & 31)) & 1u; }

__global__ __launch_bounds__(256) void ctrl_llr(CtrlArgs a)
{
  const CtrlJob& J = a.jobs ? a.jobs[blockIdx.x] : a.inl;
  __shared__ float    s_llr[32];
  __shared__ uint32_t s_cfi;
  const float         noise = J.d_noise ? *J.d_noise : J.noise;
  const uint32_t      t     = threadIdx.x;
  const uint32_t*     pcs   = a.pcfich_seq + J.sf_idx;
  // PCFICH (16 symbols: 16 / 8 / 4 work items for 1 / 2 / 4 ports)
  if (a.nof_ports == 1 && t < 16) {
    const float2 l = demod(eq_single(a, J, a.pcfich_re[t], noise), (*pcs >> (2 * t)) & 1u, (*pcs >> (2 * t + 1)) & 1u);
    s_llr[2 * t] = l.x, s_llr[2 * t + 1] = l.y;
  } else if (a.nof_ports == 2 && t < 8) {
    float2 d0, d1;
    eq_pair(a, J, a.pcfich_re[2 * t], a.pcfich_re[2 * t + 1], false, d0, d1);
    const float2 l0 = demod(d0, (*pcs >> (4 * t)) & 1u, (*pcs >> (4 * t + 1)) & 1u);
    const float2 l1 = demod(d1, (*pcs >> (4 * t + 2)) & 1u, (*pcs >> (4 * t + 3)) & 1u);
    s_llr[4 * t] = l0.x, s_llr[4 * t + 1] = l0.y, s_llr[4 * t + 2] = l1.x, s_llr[4 * t + 3] = l1.y;
  } else if (a.nof_ports == 4 && t < 4) {
    float2 d[4];
    eq_quad(a, J, a.pcfich_re + 4 * t, d);
    for (int q = 0; q < 4; q++) {
      const uint32_t i = 4 * t + q;
      const float2   l = demod(d[q], (*pcs >> (2 * i)) & 1u, (*pcs >> (2 * i + 1)) & 1u);
      s_llr[2 * i] = l.x, s_llr[2 * i + 1] = l.y;
    }
  }
  __syncthreads();
  if (t == 0) {
    // correlation with the CFI code words (36.212 Table 5.3.4-1: 011 / 101 / 110 repeated), first maximum wins,
    // CFI 1 when no correlation is positive (srslte_pcfich_cfi_decode)
    const uint32_t w[3] = {0x6u, 0x5u, 0x3u}; // bit b of w = code bit j with j % 3 == b
    float          best = 0.f;
    uint32_t       cfi  = 1;
    for (uint32_t q = 0; q < 3; q++) {
      float s = 0.f;
      for (uint32_t j = 0; j < 32; j++) s += (((w[q] >> (j % 3)) & 1u) ? 1.f : -1.f) * s_llr[j];
      a.corr[3 * blockIdx.x + q] = s;
      if (s > best) {
        best = s;
        cfi  = q + 1;
      }
    }
    a.cfi[blockIdx.x] = cfi;
    s_cfi             = cfi;
  }
  __syncthreads();
  // PDCCH region of the decoded CFI
  const uint32_t  cfi  = s_cfi;
  const uint32_t  n    = 4 * a.nregs[cfi - 1];
  const uint32_t* re   = a.pdcch_re + (size_t)(cfi - 1) * PDCCH_MAX_REGS * 4;
  const uint32_t* seq  = a.pdcch_seq + (size_t)J.sf_idx * a.seq_words;
  float*          out  = a.llr + (size_t)blockIdx.x * a.llr_stride;
  const float     nz   = noise / 2;
  if (a.nof_ports == 1) {
    for (uint32_t i = t; i < n; i += blockDim.x) {
      const float2 l = demod(eq_single(a, J, re[i], nz), seq_bit(seq, 2 * i), seq_bit(seq, 2 * i + 1));
      reinterpret_cast<float2*>(out)[i] = l;
    }
  } else if (a.nof_ports == 2) {
    const uint32_t nsse = n > 32 ? 4 * (n / 4) : 0;
    for (uint32_t i = t; i < n / 2; i += blockDim.x) {
      float2 d0, d1;
      eq_pair(a, J, re[2 * i], re[2 * i + 1], 2 * i < nsse, d0, d1);
      const float2 l0 = demod(d0, seq_bit(seq, 4 * i), seq_bit(seq, 4 * i + 1));
      const float2 l1 = demod(d1, seq_bit(seq, 4 * i + 2), seq_bit(seq, 4 * i + 3));
      reinterpret_cast<float4*>(out)[i] = make_float4(l0.x, l0.y, l1.x, l1.y);
    }
  } else {
    for (uint32_t i = t; i < n / 4; i += blockDim.x) {
      float2 d[4];
      eq_quad(a, J, re + 4 * i, d);
      for (int q = 0; q < 4; q++) {
        const uint32_t k = 4 * i + q;
        reinterpret_cast<float2*>(out)[k] = demod(d[q], seq_bit(seq, 2 * k), seq_bit(seq, 2 * k + 1));
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ blind decoding

// one wave per workgroup: most candidates fail the mean-|LLR| gate at once while a decoding wave runs a long serial
// trellis, and a workgroup's LDS is released only when all its waves are done -- with 4 waves per workgroup a CU held
// 5 workgroups (LDS-bound) whatever few of their waves were decoding
constexpr uint32_t WAVES   = 1;
static_assert((PDCCH_SLOTS * PDCCH_FMTS) % WAVES == 0, "a workgroup never straddles two subframes' tail");

// candidate location of a slot (pdcch.c:230-330), computed uniformly by every lane; false: no candidate there
__device__ __forceinline__ bool slot_location(const BlindJob& bj, uint32_t slot, uint32_t ntot, uint32_t& L,
                                              uint32_t& ncce)
{
  const uint32_t space = slot < MI355_MAX_CANDIDATES_UE ? 0u : 1u;
  const uint32_t cidx  = space ? slot - MI355_MAX_CANDIDATES_UE : slot;
  uint32_t       k     = 0;
  if (space == 0) {
    // pdcch.c:230-290 without the candidate list: within a level, candidate i repeats an earlier one exactly when
    // i >= N / L (the modulo wraps), and candidates of different levels never coincide, so level l contributes
    // min(6/6/2/2, N / L) candidates in order
    for (uint32_t l = 0; l < 4; l++) {
      const uint32_t LL = 1u << l, m = ntot / LL, cnt = min(l < 2 ? 6u : 2u, m);
      if (cidx < k + cnt) {
        L = l, ncce = LL * ((bj.Yk + (cidx - k)) % m);
        return true;
      }
      k += cnt;
    }
  } else {
    for (uint32_t l = 2; l <= 3; l++) {
      const uint32_t LL = 1u << l;
      for (uint32_t i = 0; i < min(ntot, 16u) / LL; i++)
        if (k < MI355_MAX_CANDIDATES_COM && LL * i + LL <= ntot) {
          if (k == cidx) {
            L = l, ncce = LL * i;
            return true;
          }
          k++;
        }
    }
  }
  return false;
}

// srslte_pdcch_decode_msg's gate (pdcch.c:392-397): mean |llr| > 0.3, the sum in double
__device__ __forceinline__ bool gate_pass(const float* llr, uint32_t E)
{
  double s = 0;
  for (uint32_t i = __lane_id(); i < E; i += 64) s += (double)fabsf(llr[i]);
  s = wave_sum(s);
  return s / E > 0.3;
}

// One wave per (subframe, search-space candidate, DCI size): every candidate that passes the gate is decoded and the
// host replays dci_blind_search over the results.  (A sequential walk -- one wave per subframe decoding only what
// dci_blind_search reaches -- was measured and dropped: 255 vs 121 us per 1,024 subframes.  A hit at level 0 or 1
// allocates a width of 0 or 1 CCE in the reference's overlap test, so little is skipped, and one serial decode chain
// per SIMD leaves the VALU idle.)
__global__ __launch_bounds__(64 * WAVES) void pdcch_blind(BlindArgs a)
{
  __shared__ WaveLds lds[WAVES];
  const uint32_t     lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint32_t     gw   = blockIdx.x * WAVES + wv;
  const uint32_t     job  = gw / (PDCCH_SLOTS * PDCCH_FMTS);
  const uint32_t     slot = (gw / PDCCH_FMTS) % PDCCH_SLOTS, fmt = gw % PDCCH_FMTS;
  DciCand*           out  = a.out + gw;
  const BlindJob&    bj   = a.jobs ? a.jobs[job] : a.inl; // read in place (a private copy indexed by space / fmt would go to scratch)
  const uint32_t     space = slot < MI355_MAX_CANDIDATES_UE ? 0u : 1u;
  const uint32_t     nbits = bj.nbits[space][fmt];
  const uint32_t     cfi   = a.cfi[job];
  const uint32_t     ntot  = (cfi >= 1 && cfi <= 3) ? a.ncce[cfi - 1] : 0u;
  uint32_t           L = 0, ncce = 0;
  if (!((bj.spaces >> space) & 1u) || !nbits || !slot_location(bj, slot, ntot, L, ncce)) {
    if (lane == 0) out->status = 0;
    return;
  }
  const uint32_t E   = 72u << L;
  const float*   llr = a.llr + (size_t)job * a.llr_stride + 72 * ncce;
  if (!gate_pass(llr, E)) {
    if (lane == 0) out->status = 1, out->L = L, out->ncce = ncce;
    return;
  }
  if (BLIND_DIAG == 1) return;
  uint32_t w0;
  decode_cand(lds[wv], llr, E, nbits, L, ncce, out, w0);
}

// Inspection (mi355_debug_conv_decode_batch): one wave per job through the routines the product kernels call.
// Mode 0 is pdcch_blind from its gate on, mode 1 pbch_decode from its decode_cand<true> on (the vector in LDS).
__global__ __launch_bounds__(64) void conv_decode_debug(const ConvDebugJob* jobs, const float* llr, DciCand* out)
{
  __shared__ WaveLds lds;
  __shared__ float   s_vec[CONV_DEBUG_MAX_E_LDS];
  const uint32_t     lane = threadIdx.x;
  const ConvDebugJob J    = jobs[blockIdx.x];
  const float*       in   = llr + J.off;
  DciCand*           o    = out + blockIdx.x;
  uint32_t           w0;
  if (J.mode == 0) {
    if (!gate_pass(in, J.E)) {
      if (lane == 0) o->status = 1, o->L = 0, o->ncce = 0;
      return;
    }
    decode_cand(lds, in, J.E, J.nbits, 0, 0, o, w0);
  } else {
    for (uint32_t j = lane; j < J.E && j < CONV_DEBUG_MAX_E_LDS; j += 64) s_vec[j] = in[j];
    __syncthreads();
    decode_cand<true>(lds, s_vec, min(J.E, CONV_DEBUG_MAX_E_LDS), J.nbits, 0, 0, o, w0, J.scale);
  }
}

} // namespace

hipError_t ctrl_launch_conv_debug(const ConvDebugJob* jobs, const float* llr, DciCand* out, uint32_t njobs,
                                  hipStream_t s)
{
  if (!njobs) return hipSuccess;
  hipLaunchKernelGGL(conv_decode_debug, dim3(njobs), dim3(64), 0, s, jobs, llr, out);
  return hipGetLastError();
}

hipError_t ctrl_launch_llr(const CtrlArgs& a, uint32_t njobs, hipStream_t s)
{
  if (!njobs) return hipSuccess;
  hipLaunchKernelGGL(ctrl_llr, dim3(njobs), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t ctrl_launch_blind(const BlindArgs& a, uint32_t njobs, hipStream_t s)
{
  if (!njobs) return hipSuccess;
  const uint32_t waves = njobs * PDCCH_SLOTS * PDCCH_FMTS;
  hipLaunchKernelGGL(pdcch_blind, dim3((waves + WAVES - 1) / WAVES), dim3(64 * WAVES), 0, s, a);
  return hipGetLastError();
}

// one wave per subframe: lane k checks candidate k (slot k / PDCCH_FMTS, format slot k % PDCCH_FMTS); the matching
// ones (decoded, CRC remainder = the searched RNTI: the only candidates dci_blind_search acts on, ue_dl.c:480-484)
// are written in slot order by their rank in the wave's ballot
__global__ __launch_bounds__(256) void pdcch_compact(CompactArgs a, uint32_t njobs)
{
  constexpr uint32_t NC = PDCCH_SLOTS * PDCCH_FMTS;
  static_assert(NC <= 64, "one candidate per lane");
  const uint32_t job  = blockIdx.x * 4 + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63;
  if (job >= njobs) return;
  const DciCand* c   = a.cand + (size_t)job * NC;
  const uint32_t rnti = a.jobs ? a.jobs[job].rnti : a.inl.rnti;
  bool           hit  = false;
  if (lane < NC) hit = c[lane].status == 2 && c[lane].crc_rem == rnti;
  const uint64_t mask = __builtin_amdgcn_ballot_w64(hit);
  DciHits*       h    = a.hits + job;
  uint32_t       b[4] = {0u, 0u, 0u, 0u};
  if (hit) {
#pragma unroll
    for (int w = 0; w < 4; w++) b[w] = c[lane].bits[w];
  }
  // distinct payloads in slot order: the first unassigned hit's bits, every hit with the same bits joins it
  uint64_t rem = mask;
  uint32_t np = 0, mine = 0;
  while (rem) { // wave-uniform
    const int      f = __builtin_ctzll(rem);
    const uint32_t f0 = __builtin_amdgcn_readlane(b[0], f), f1 = __builtin_amdgcn_readlane(b[1], f);
    const uint32_t f2 = __builtin_amdgcn_readlane(b[2], f), f3 = __builtin_amdgcn_readlane(b[3], f);
    const bool     same = hit && b[0] == f0 && b[1] == f1 && b[2] == f2 && b[3] == f3;
    if (same) mine = np;
    if ((int)lane == f && np < PDCCH_HPAY) {
#pragma unroll
      for (int w = 0; w < 4; w++) h->bits[np][w] = b[w];
    }
    np++;
    rem &= ~__builtin_amdgcn_ballot_w64(same);
  }
  if (lane == 0) {
    h->n    = (uint32_t)__builtin_popcountll(mask);
    h->npay = np;
  }
  if (hit) {
    const uint32_t rank = (uint32_t)__builtin_popcountll(mask & ((1ull << lane) - 1));
    if (rank < PDCCH_HMAX) {
      h->slot[rank] = (uint8_t)lane;
      h->pidx[rank] = (uint8_t)mine;
    }
  }
}

hipError_t ctrl_launch_compact(const CompactArgs& a, uint32_t njobs, hipStream_t s)
{
  if (!njobs) return hipSuccess;
  hipLaunchKernelGGL(pdcch_compact, dim3((njobs + 3) / 4), dim3(256), 0, s, a, njobs);
  return hipGetLastError();
}

} // namespace mi355
