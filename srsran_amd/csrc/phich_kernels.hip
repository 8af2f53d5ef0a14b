// srsran_amd/csrc/phich_kernels.hip -- PHICH decoding on gfx950 (srslte_phich_decode, phich.c:183-315).
//
//   phich_decode  4 lanes per job, 16 jobs per wave.  Lanes 0..2 of a job own one ACK bit each: the four REs of one
//                 REG, which is one SFBC pair twice (2 ports) or one 4-symbol group (4 ports), so a lane equalises its
//                 REG without another lane's symbols.  It applies the +-1 scrambling sequence, despreads with the
//                 job's four-chip sequence and demaps BPSK; the three soft bits meet in lane 0 through lane shuffles,
//                 lane 0 correlates them with the two code words and writes the 8-byte result.  No LDS, no atomics.
//
// A dozen REs per job: nothing here is GEMM-shaped, the work is the gather.  The equalisers (ctrl_eq.h) evaluate the
// reference's formulas without FMA contraction (built with -ffp-contract=off), and every operation after them follows
// phich.c / demod_soft.c in order, so ack_value and distance equal the reference's bit for bit.
#include <hip/hip_runtime.h>

#include "ctrl_eq.h"
#include "pdcch_internal.h"

namespace mi355 {

namespace {

constexpr uint32_t PHICH_LANES = 4;   // per job (the fourth lane idles: a power of two keeps a job inside one wave)
constexpr uint32_t PHICH_BLOCK = 256; // 64 jobs per workgroup

__global__ __launch_bounds__(PHICH_BLOCK) void phich_decode(PhichArgs a)
{
  const uint32_t t = blockIdx.x * PHICH_BLOCK + threadIdx.x;
  const uint32_t job = t / PHICH_LANES, bit = t % PHICH_LANES;
  // every lane stays to the end (the shuffles below read lanes 1 and 2 of each job); lanes past the job count or the
  // third bit load nothing
  const bool act = job < a.njobs && bit < 3;
  float      soft = 0.f;
  if (act) {
    const PhichJob  pj = a.jobs[job];
    const CtrlJob&  J  = a.sfs[pj.sf];
    const uint32_t* re = a.re + (size_t)pj.ngroup * 12 + 4 * bit;
    CtrlArgs        ca{}; // what the shared equalisers read of it
    ca.nof_rx = a.nof_rx;
    ca.ce_row = a.ce_row;
    const uint32_t r[4] = {re[0], re[1], re[2], re[3]};
    float2         d[4];
    if (a.nof_ports == 1) {
      const float noise = J.d_noise ? *J.d_noise : J.noise;
      for (int q = 0; q < 4; q++) d[q] = eq_single(ca, J, r[q], noise);
    } else if (a.nof_ports == 2) {
      // 12 symbols are below the reference's SSE threshold (n > 32): diversity_gen_ for every pair
      eq_pair(ca, J, r[0], r[1], false, d[0], d[1]);
      eq_pair(ca, J, r[2], r[3], false, d[2], d[3]);
    } else {
      eq_quad(ca, J, r, d);
    }
    // srslte_scrambling_c: the symbol times the +-1 sequence; despreading (phich.c:296-301):
    // z += conj(w[nseq][j]) * d[4 bit + j] / 4, j = 0..3 from zero.  w is +-1 (nseq < 4) or +-j (36.211 Table 6.9.1-2):
    // conj(j) d = d.im - j d.re
    const uint32_t c  = a.seq[J.sf_idx] >> (4 * bit);
    const uint32_t wm = (0x6CA0u >> (4 * (pj.nseq & 3))) & 15u; // bit j set: chip j of {++++, +-+-, ++--, +--+} is -1
    float          zr = 0.f, zi = 0.f;
    for (int j = 0; j < 4; j++) {
      const float sc = ((c >> j) & 1u) ? -1.f : 1.f;
      const float xr = d[j].x * sc, xi = d[j].y * sc;
      const float w  = ((wm >> j) & 1u) ? -1.f : 1.f;
      if (pj.nseq < 4) {
        zr += (w * xr) / 4.f;
        zi += (w * xi) / 4.f;
      } else {
        zr += (w * xi) / 4.f;
        zi += (-w * xr) / 4.f;
      }
    }
    // demod_bpsk_lte (demod_soft.c:125-130): the product with M_SQRT1_2 in double
    soft = (float)((double)(-(zr + zi)) * 0.70710678118654752440);
  }
  const float b1 = __shfl_down(soft, 1), b2 = __shfl_down(soft, 2);
  if (job < a.njobs && bit == 0) {
    // srslte_phich_ack_decode (phich.c:149-173): dot products with {-1,-1,-1} and {1,1,1} over 3, the first above
    // -9999 and then any larger one wins; a NaN soft bit exceeds nothing (the reference leaves distance unwritten)
    const float corr[2] = {((0.f + -1.f * soft) + -1.f * b1 + -1.f * b2) / 3.f, ((0.f + soft) + b1 + b2) / 3.f};
    float       best = -9999.f, dist = 0.f;
    uint32_t    ack  = 0;
    for (uint32_t i = 0; i < 2; i++)
      if (corr[i] > best) {
        best = corr[i];
        dist = best;
        ack  = i;
      }
    a.out[job] = PhichOut{ack, dist};
  }
}

} // namespace

hipError_t phich_launch_decode(const PhichArgs& a, hipStream_t s)
{
  if (!a.njobs) return hipSuccess;
  const uint32_t blocks = (a.njobs * PHICH_LANES + PHICH_BLOCK - 1) / PHICH_BLOCK;
  hipLaunchKernelGGL(phich_decode, dim3(blocks), dim3(PHICH_BLOCK), 0, s, a);
  return hipGetLastError();
}

} // namespace mi355
