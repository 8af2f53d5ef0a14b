// srsran_amd/csrc/sync_kernels.hip -- cell search (srslte_sync_find) on gfx950.
//
//   sync_corr      one workgroup per (tile of 256 correlation outputs, job): the input tile and its fft_size - 1 halo
//                  staged once in LDS, the conjugated time-domain PSS replicas staged 128 taps at a time, every
//                  configured N_id_2 hypothesis from that one read: the direct-form correlation with the reference's
//                  output indexing (linear convolution of the window, or the sliding dot product of pss.c:491-496
//                  for windows shorter than the FFT), taps summed in double and stored as float, |.|^2 and, for
//                  independent jobs, the average against a zero state (pss.c:498-509).
//   sync_ema_scan  SEQUENCE: the same average run over the jobs of the call against the object's conv_output_avg.
//   sync_peak      one workgroup per (hypothesis, job): argmax (first index on ties), compute_peak_sidelobe as
//                  written (pss.c:413-442), the threshold, the PSS filter as a 62-bin DFT and its inverse
//                  (pss.c:594-609), the CFO estimate (pss.c:616-640) and the raw CP metrics (sync.c:452-491).
//   sync_scan      cfo_pss_mean with its 7 kHz rule, the CP metrics' averages and the CP decision, scanned over the
//                  jobs of a sequence (one thread per hypothesis) or per job for independent ones.
//   sync_sss       one workgroup per (hypothesis, job): per frame-type trial the CFO rotation of the SSS symbol, its
//                  62 central DFT bins, extract_pair_sss, the m0 / m1 correlations of the chosen algorithm
//                  (find_sss.c:67-192), the N_id_1 lookup, then the choice between the trials (sync.c:795-819) and
//                  the result record.
//
// Built with -ffp-contract=off: the averages and metrics follow the reference's formulas operation by operation.
#include <hip/hip_runtime.h>

#include "sync_internal.h"

namespace mi355 {

namespace {

__device__ inline float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ inline float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }

// sum over the 256 threads of a block; every thread gets the result
__device__ inline float block_sum(float v, float* red)
{
  const uint32_t t = threadIdx.x;
  __syncthreads();
  red[t] = v;
  __syncthreads();
  for (uint32_t s = 128; s > 0; s >>= 1) {
    if (t < s) red[t] += red[t + s];
    __syncthreads();
  }
  return red[0];
}

__global__ __launch_bounds__(SYNC_TILE) void sync_corr(SyncArgs a)
{
  extern __shared__ float2 xs[];                     // [SYNC_TILE + fft - 1] input tile + halo
  __shared__ float2        hs[SYNC_HYPS][SYNC_TAPS]; // replica taps of this pass
  const uint32_t t = threadIdx.x, job = blockIdx.y, i0 = blockIdx.x * SYNC_TILE, M = a.fft;
  const SyncJob  J    = a.jobs[job];
  const float2*  x    = J.in + J.find_offset;
  const uint32_t span = SYNC_TILE + M - 1;
  // long windows: out[i] = sum_k h[k] x[i - k], x = 0 outside [0, N); short ones: out[i] = sum_k h[k] x[i + k]
  const int      base  = a.shortwin ? (int)i0 : (int)i0 - (int)(M - 1);
  const uint32_t limit = a.shortwin ? a.N + M - 1 : a.N;
  for (uint32_t j = t; j < span; j += SYNC_TILE) {
    const int idx = base + (int)j;
    xs[j]         = idx >= 0 && (uint32_t)idx < limit ? x[idx] : make_float2(0.f, 0.f);
  }
  // The taps are summed in double: a product of two floats is exact there, so a 128 .. 2048-tap sum carries one
  // rounding when it is stored as float, like an output of the reference's transform, not one per tap.
  double accr[SYNC_HYPS], acci[SYNC_HYPS];
  for (uint32_t h = 0; h < SYNC_HYPS; h++) accr[h] = 0.0, acci[h] = 0.0;
  for (uint32_t k0 = 0; k0 < M; k0 += SYNC_TAPS) {
    __syncthreads();
    const uint32_t nt = min(SYNC_TAPS, M - k0);
    for (uint32_t j = t; j < a.nhyp * SYNC_TAPS; j += SYNC_TILE) {
      const uint32_t h = j / SYNC_TAPS, k = j % SYNC_TAPS;
      if (k < nt) hs[h][k] = a.pss_time[(size_t)(a.hyp0 + h) * M + k0 + k];
    }
    __syncthreads();
    for (uint32_t k = 0; k < nt; k++) {
      const float2 v = a.shortwin ? xs[t + k0 + k] : xs[t + (M - 1) - (k0 + k)];
      const double vr = v.x, vi = v.y;
      for (uint32_t h = 0; h < SYNC_HYPS; h++)
        if (h < a.nhyp) {
          const double hr = hs[h][k].x, hi = hs[h][k].y;
          accr[h] += hr * vr - hi * vi;
          acci[h] += hr * vi + hi * vr;
        }
    }
  }
  const uint32_t i = i0 + t;
  if (i >= a.L) return;
  const bool ema = a.cfg.ema_alpha < 1.0f && a.cfg.ema_alpha > 0.0f;
  for (uint32_t h = 0; h < a.nhyp; h++) {
    float v = 0.f;
    if (i < a.nout) {
      const float cr = (float)accr[h], ci = (float)acci[h]; // conv_output is float
      v              = cr * cr + ci * ci;
      if (ema && !a.seq) v = v * a.cfg.ema_alpha + 0.f * (1 - a.cfg.ema_alpha);
    }
    a.avg[((size_t)job * a.nhyp + h) * a.L + i] = v;
  }
}

__global__ __launch_bounds__(256) void sync_ema_scan(SyncArgs a)
{
  const uint32_t i = blockIdx.x * 256 + threadIdx.x, h = blockIdx.y;
  if (i >= a.L) return;
  const bool ema  = a.cfg.ema_alpha < 1.0f && a.cfg.ema_alpha > 0.0f;
  float      prev = a.avg_state[(size_t)h * a.L + i];
  if (i < a.nout)
    for (uint32_t job = 0; job < a.njobs; job++) {
      float*      p = a.avg + ((size_t)job * a.nhyp + h) * a.L + i;
      const float v = *p;
      prev          = ema ? v * a.cfg.ema_alpha + prev * (1 - a.cfg.ema_alpha) : v;
      *p            = prev;
    }
  a.avg_state[(size_t)h * a.L + i] = prev;
}

__global__ __launch_bounds__(256) void sync_peak(SyncArgs a)
{
  extern __shared__ float2 sm[]; // [fft] the PSS symbol (filtered or not) | [62] bins
  __shared__ float         red[256];
  __shared__ uint32_t      redi[256];
  __shared__ int           s_lb, s_ub;
  const uint32_t t = threadIdx.x, h = blockIdx.x, job = blockIdx.y, M = a.fft;
  const float*   avg = a.avg + ((size_t)job * a.nhyp + h) * a.L;
  const SyncJob  J   = a.jobs[job];
  // srslte_vec_max_fi over conv_output_len - 1 values, first index on ties
  float    bv = -INFINITY;
  uint32_t bi = 0xFFFFFFFFu;
  for (uint32_t i = t; i < a.nout; i += 256) {
    const float v = avg[i];
    if (v > bv) bv = v, bi = i;
  }
  red[t] = bv, redi[t] = bi;
  __syncthreads();
  for (uint32_t s = 128; s > 0; s >>= 1) {
    if (t < s && (red[t + s] > red[t] || (red[t + s] == red[t] && redi[t + s] < redi[t])))
      red[t] = red[t + s], redi[t] = redi[t + s];
    __syncthreads();
  }
  const uint32_t p     = redi[0] == 0xFFFFFFFFu ? 0u : redi[0]; // (no value compares greater: index 0, as the scalar loop)
  const float    pkabs = avg[p];
  __syncthreads();
  // compute_peak_sidelobe: the walk down both flanks of the main lobe, then the larger of the two side maxima
  float psr = 0.f;
  if (a.cfg.threshold > 0.f) {
    const int len = (int)a.nout + 1; // conv_output_len
    if (t == 0) {
      int ub = (int)p + 1;
      while (avg[ub + 1] <= avg[ub] && ub < len) ub++;
      int lb = 0;
      if (p > 2) {
        lb = (int)p - 1;
        while (avg[lb - 1] <= avg[lb] && lb > 1) lb--;
      }
      s_ub = ub, s_lb = lb;
    }
    __syncthreads();
    const int ub = s_ub, lb = s_lb;
    int       dr = len - 1 - ub;
    if (dr < 0) dr = 0;
    float mr = dr > 0 ? -INFINITY : avg[ub], ml = lb > 0 ? -INFINITY : avg[0];
    for (int i = (int)t; i < dr; i += 256) mr = fmaxf(mr, avg[ub + i]);
    for (int i = (int)t; i < lb; i += 256) ml = fmaxf(ml, avg[i]);
    red[t] = mr;
    __syncthreads();
    for (uint32_t s = 128; s > 0; s >>= 1) {
      if (t < s) red[t] = fmaxf(red[t], red[t + s]);
      __syncthreads();
    }
    mr = red[0];
    __syncthreads();
    red[t] = ml;
    __syncthreads();
    for (uint32_t s = 128; s > 0; s >>= 1) {
      if (t < s) red[t] = fmaxf(red[t], red[t + s]);
      __syncthreads();
    }
    ml = red[0];
    __syncthreads();
    psr = pkabs / (mr > ml ? mr : ml);
  }
  const uint32_t peak_pos = a.shortwin ? p + M : p;
  const bool     found    = psr >= a.cfg.threshold || a.cfg.threshold == 0.f;
  const uint32_t pp       = peak_pos + J.find_offset;
  const uint32_t cp_ext   = sync_cp_len(M, 512), cp_norm = sync_cp_len(M, 144);
  const bool     space    = pp >= 2 * (M + cp_ext);

  // PSS-based CFO
  float cfo       = 0.f;
  bool  cfo_valid = found && a.cfg.cfo_pss_enable && peak_pos >= M;
  if (cfo_valid) {
    const float2* x  = J.in + pp - M;
    float2*       X  = sm + M;
    for (uint32_t n = t; n < M; n += 256) sm[n] = x[n];
    __syncthreads();
    if (a.cfg.pss_filt_enable) {
      if (t < 62) {
        const uint32_t k   = (uint32_t)(central_bin(t) + (int)M) % M;
        float2         acc = make_float2(0.f, 0.f);
        for (uint32_t n = 0; n < M; n++) acc = cadd(acc, cmul(sm[n], a.tw[(k * n) % M]));
        X[t] = acc;
      }
      __syncthreads();
      for (uint32_t n = t; n < M; n += 256) {
        float2 acc = make_float2(0.f, 0.f);
        for (uint32_t b = 0; b < 62; b++) {
          const uint32_t k = (uint32_t)(central_bin(b) + (int)M) % M;
          const float2   w = a.tw[(k * n) % M];
          acc              = cadd(acc, cmul(X[b], make_float2(w.x, -w.y)));
        }
        sm[n] = acc; // (the spectrum is in X: sm is no longer read)
      }
      __syncthreads();
    }
    const float2* hpss = a.pss_time + (size_t)(a.hyp0 + h) * M;
    float2        y0 = make_float2(0.f, 0.f), y1 = y0;
    for (uint32_t n = t; n < M / 2; n += 256) {
      y0 = cadd(y0, cmul(hpss[n], sm[n]));
      y1 = cadd(y1, cmul(hpss[M / 2 + n], sm[M / 2 + n]));
    }
    const float y0r = block_sum(y0.x, red), y0i = block_sum(y0.y, red);
    const float y1r = block_sum(y1.x, red), y1i = block_sum(y1.y, red);
    const float2 pr = cmul(make_float2(y0r, -y0i), make_float2(y1r, y1i));
    cfo             = (float)((double)atan2f(pr.y, pr.x) / M_PI);
  }

  // srslte_sync_detect_cp's correlations; the averages and the decision belong to the scan
  float    m_norm = 0.f, m_ext = 0.f;
  uint32_t r_gt = 0;
  if (found && space && a.cfg.detect_cp) {
    // (space: pp >= 2 (M + cp_ext), so nof_symbols is 2 or 3 and the reference's nof_symbols == 0 branch cannot be taken)
    uint32_t nsym = pp / (M + cp_ext);
    if (nsym > 3) nsym = 3;
    {
      const float2* xn = J.in + pp - nsym * (M + cp_norm);
      const float2* xe = J.in + pp - nsym * (M + cp_ext);
      float rn = 0.f, cn = 0.f, re = 0.f, ce = 0.f;
      for (uint32_t s = 0; s < nsym; s++) {
        float r = 0.f, c = 0.f;
        for (uint32_t n = t; n < cp_norm; n += 256) {
          const float2 u = xn[s * (M + cp_norm) + M + n], v = xn[s * (M + cp_norm) + n];
          r += u.x * v.x + u.y * v.y;
          c += v.x * v.x + v.y * v.y;
        }
        rn += block_sum(r, red);
        cn += (float)cp_norm * (block_sum(c, red) / (float)cp_norm);
        r = 0.f, c = 0.f;
        for (uint32_t n = t; n < cp_ext; n += 256) {
          const float2 u = xe[s * (M + cp_ext) + M + n], v = xe[s * (M + cp_ext) + n];
          r += u.x * v.x + u.y * v.y;
          c += v.x * v.x + v.y * v.y;
        }
        re += block_sum(r, red);
        ce += (float)cp_ext * (block_sum(c, red) / (float)cp_ext);
      }
      m_norm   = (cn > 0.f ? rn / cn : 0.f) / (float)nsym;
      m_ext    = (ce > 0.f ? re / ce : 0.f) / (float)nsym;
      r_gt     = rn > re;
    }
  }
  if (t == 0) {
    const size_t      o = (size_t)job * a.nhyp + h;
    mi355_sync_res_t& R = a.res[o];
    R.ret               = !found ? MI355_SYNC_NOFOUND : space ? MI355_SYNC_FOUND : MI355_SYNC_FOUND_NOSPACE;
    R.n_id_2            = a.hyp0 + h;
    R.peak_pos          = peak_pos;
    R.peak_value        = psr;
    R.peak_abs          = pkabs;
    R.cfo_pss           = cfo;
    SyncRec& C          = a.rec[o];
    C.found = found, C.space = space, C.cfo_valid = cfo_valid;
    C.m_norm = m_norm, C.m_ext = m_ext, C.r_norm_gt = r_gt; // (cp_in: the scan's)
  }
}

// one call's share of srslte_sync_find's scalar state
__device__ inline void scan_step(const SyncArgs& a, SyncState& S, SyncRec& C, mi355_sync_res_t& R)
{
  if (C.cfo_valid) {
    if (!S.cfo_pss_is_set) {
      S.cfo_pss_mean   = R.cfo_pss;
      S.cfo_pss_is_set = 1;
    } else if (15000 * fabsf(R.cfo_pss) < 7000) {
      S.cfo_pss_mean = a.cfg.cfo_ema_alpha * R.cfo_pss + (1 - a.cfg.cfo_ema_alpha) * S.cfo_pss_mean;
    }
  }
  R.cfo_pss_mean = S.cfo_pss_mean;
  C.cp_in        = S.cp;
  if (C.found && C.space && a.cfg.detect_cp) {
    // CP_EMA_ALPHA is a double constant: the average is formed in double
    S.M_norm_avg = (float)(0.1 * (double)C.m_norm + (1 - 0.1) * (double)S.M_norm_avg);
    S.M_ext_avg  = (float)(0.1 * (double)C.m_ext + (1 - 0.1) * (double)S.M_ext_avg);
    if (S.M_norm_avg > S.M_ext_avg) S.cp = MI355_CP_NORM;
    else if (S.M_norm_avg < S.M_ext_avg) S.cp = MI355_CP_EXT;
    else S.cp = C.r_norm_gt ? MI355_CP_NORM : MI355_CP_EXT;
  }
  R.cp         = S.cp;
  R.M_norm_avg = S.M_norm_avg;
  R.M_ext_avg  = S.M_ext_avg;
}

__global__ __launch_bounds__(64) void sync_scan(SyncArgs a)
{
  const uint32_t g = blockIdx.x * 64 + threadIdx.x;
  if (a.seq) {
    if (g >= a.nhyp) return;
    SyncState S = a.state[g];
    for (uint32_t job = 0; job < a.njobs; job++) scan_step(a, S, a.rec[(size_t)job * a.nhyp + g], a.res[(size_t)job * a.nhyp + g]);
    a.state[g] = S;
  } else {
    if (g >= a.njobs * a.nhyp) return;
    SyncState S{};
    S.cp = a.cfg.cp;
    scan_step(a, S, a.rec[g], a.res[g]);
  }
}

// corr_all_sz_partial / corr_all_zs for one m: |sum z s|^2 per part
__device__ inline float sss_corr_m(const float2* z, const float* s, uint32_t parts, uint32_t nm)
{
  float out = 0.f;
  for (uint32_t j = 0; j < parts; j++) {
    float2 acc = make_float2(0.f, 0.f);
    for (uint32_t i = 0; i < nm; i++) acc = make_float2(acc.x + z[j * nm + i].x * s[j * nm + i], acc.y + z[j * nm + i].y * s[j * nm + i]);
    const float v = acc.x * acc.x + acc.y * acc.y;
    out           = j == 0 ? v : v + out;
  }
  return out;
}

__device__ inline uint32_t argmax31(const float* v)
{
  uint32_t b = 0;
  for (uint32_t i = 1; i < SSS_N; i++)
    if (v[i] > v[b]) b = i;
  return b;
}

__global__ __launch_bounds__(64) void sync_sss(SyncArgs a)
{
  extern __shared__ float2 xr[]; // [fft] the rotated SSS symbol
  __shared__ float2        y[2][SSS_N], yp[SSS_N];
  __shared__ float         corr[SSS_N];
  __shared__ uint32_t      s_m0;
  const uint32_t t = threadIdx.x, h = blockIdx.x, job = blockIdx.y, M = a.fft, id2 = a.hyp0 + h;
  const size_t   o = (size_t)job * a.nhyp + h;
  const SyncJob  J = a.jobs[job];
  mi355_sync_res_t& R = a.res[o];
  const SyncRec  C    = a.rec[o];
  // reset values of what this call may not compute
  uint32_t avail = 0, detected = 0, m0o = 0, m1o = 0, nid1 = N_ID_1_NONE, sf = 0, ftype = a.cfg.frame_type;
  float    m0v = 0.f, m1v = 0.f, scorr = 0.f;
  if (C.found && C.space && a.cfg.sss_en) {
    const uint32_t ntr = a.cfg.detect_frame_type ? 2u : 1u;
    uint32_t       t_sf[2] = {0, 0}, t_id[2] = {N_ID_1_NONE, N_ID_1_NONE}, t_det[2] = {0, 0}, t_m0[2] = {0, 0}, t_m1[2] = {0, 0};
    float          t_corr[2] = {0.f, 0.f}, t_m0v[2] = {0.f, 0.f}, t_m1v[2] = {0.f, 0.f};
    avail = 1;
    uint32_t       last = 0; // the last trial that ran: q->m0 .. m1_value hold its values
    const int      symsz = (int)(M + sync_cp_sz(M, C.cp_in)), cpsz = (int)sync_cp_sz(M, C.cp_in);
    const uint32_t parts = a.cfg.sss_alg == MI355_SSS_PARTIAL_3 ? 3u : 1u, nm = SSS_N / parts;
    for (uint32_t f = 0; f < ntr; f++) {
      const uint32_t ft  = a.cfg.detect_frame_type ? f : a.cfg.frame_type;
      const int      idx = (int)J.find_offset + (int)R.peak_pos - (ft == MI355_FDD ? 2 : 4) * symsz + cpsz;
      if (idx < 0) {
        avail = 0;
        continue;
      }
      last = f;
      __syncthreads();
      const float freq = -R.cfo_pss_mean / (float)M;
      for (uint32_t n = t; n < M; n += 64) {
        float2 v = J.in[idx + n];
        if (a.cfg.cfo_pss_enable) {
          float sn, cs;
          sincosf(2.0f * (float)M_PI * freq * (float)n, &sn, &cs);
          v = cmul(v, make_float2(cs, sn));
        }
        xr[n] = v;
      }
      __syncthreads();
      if (t < 62) {
        const uint32_t k   = (uint32_t)(central_bin(t) + (int)M) % M;
        float2         acc = make_float2(0.f, 0.f);
        for (uint32_t n = 0; n < M; n++) acc = cadd(acc, cmul(xr[n], a.tw[(k * n) % M]));
        y[t & 1][t >> 1] = acc;
      }
      __syncthreads();
      if (t < 2) { // the normalisation and the c0 / c1 unmasking
        float pw = 0.f;
        for (uint32_t i = 0; i < SSS_N; i++) pw += y[t][i].x * y[t][i].x + y[t][i].y * y[t][i].y;
        pw /= (float)SSS_N;
        const float rms = pw != 0.0f ? sqrtf(pw) : 1.0f, g = (float)(1.0 / (double)rms);
        for (uint32_t i = 0; i < SSS_N; i++) {
          const float c = a.sss->c[id2][t][i];
          y[t][i]       = make_float2(y[t][i].x * g * c, y[t][i].y * g * c);
        }
      }
      __syncthreads();
      for (uint32_t half = 0; half < 2; half++) {
        if (half == 1) {
          if (t < SSS_N) {
            const float z = a.sss->z1[s_m0][t];
            y[1][t]       = make_float2(y[1][t].x * z, y[1][t].y * z);
          }
          __syncthreads();
        }
        if (a.cfg.sss_alg == MI355_SSS_DIFF) {
          if (t < SSS_N - 1) yp[t] = cmul(y[half][t + 1], make_float2(y[half][t].x, -y[half][t].y));
          __syncthreads();
          if (t < SSS_N) corr[t] = sss_corr_m(yp, a.sss->sd[t], 1, SSS_N - 1);
        } else {
          if (t < SSS_N) corr[t] = sss_corr_m(y[half], a.sss->s[t], parts, nm);
        }
        __syncthreads();
        if (t == 0) {
          const uint32_t m = argmax31(corr);
          if (half == 0) s_m0 = m, t_m0[f] = m, t_m0v[f] = corr[m];
          else t_m1[f] = m, t_m1v[f] = corr[m];
        }
        __syncthreads();
      }
      if (t == 0) {
        const uint32_t m0 = t_m0[f], m1 = t_m1[f];
        t_corr[f] = t_m0v[f] + t_m1v[f];
        t_sf[f]   = m1 > m0 ? 0u : 5u;
        if (t_corr[f] > a.cfg.sss_corr_threshold) { // srslte_sss_N_id_1 (unsigned wrap of m - 1 included)
          if (m1 > m0) {
            if (m0 < 30 && m1 - 1 < 30) t_id[f] = a.sss->n_id_1[m0][m1 - 1], t_det[f] = 1;
          } else if (m1 < 30 && m0 - 1 < 30) {
            t_id[f] = a.sss->n_id_1[m1][m0 - 1], t_det[f] = 1;
          }
        }
      }
    }
    if (t == 0) {
      uint32_t w = 0;
      detected   = t_det[0] | t_det[1];
      bool take  = true;
      if (a.cfg.detect_frame_type) {
        w     = t_corr[0] > t_corr[1] ? 0u : 1u;
        ftype = w == 0 ? MI355_FDD : MI355_TDD;
      } else {
        take = detected != 0;
      }
      if (take) {
        sf    = t_sf[w] + (ftype == MI355_TDD ? 1u : 0u);
        nid1  = t_det[w] ? t_id[w] : N_ID_1_NONE;
        scorr = t_corr[w];
      }
      m0o = t_m0[last], m1o = t_m1[last], m0v = t_m0v[last], m1v = t_m1v[last];
    }
  }
  if (t == 0) {
    R.sss_available = avail, R.sss_detected = detected;
    R.m0 = m0o, R.m1 = m1o, R.m0_value = m0v, R.m1_value = m1v, R.sss_corr = scorr;
    R.n_id_1 = nid1, R.sf_idx = sf, R.frame_type = ftype;
    R.cell_id = nid1 < 168 ? (int32_t)(nid1 * 3 + id2) : -1;
  }
}

__global__ __launch_bounds__(256) void sync_clear(float* p, size_t n, SyncState* st, uint32_t nhyp, uint32_t cp)
{
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) p[i] = 0.f;
  if (i < nhyp) {
    SyncState S{};
    S.cp  = cp;
    st[i] = S;
  }
}

} // namespace

hipError_t sync_launch_corr(const SyncArgs& a, hipStream_t s)
{
  const dim3   grid((a.L + SYNC_TILE - 1) / SYNC_TILE, a.njobs);
  const size_t lds = (size_t)(SYNC_TILE + a.fft - 1) * sizeof(float2);
  hipLaunchKernelGGL(sync_corr, grid, dim3(SYNC_TILE), lds, s, a);
  return hipGetLastError();
}

hipError_t sync_launch_ema_scan(const SyncArgs& a, hipStream_t s)
{
  hipLaunchKernelGGL(sync_ema_scan, dim3((a.L + 255) / 256, a.nhyp), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t sync_launch_peak(const SyncArgs& a, hipStream_t s)
{
  hipLaunchKernelGGL(sync_peak, dim3(a.nhyp, a.njobs), dim3(256), (size_t)(a.fft + 62) * sizeof(float2), s, a);
  return hipGetLastError();
}

hipError_t sync_launch_scan(const SyncArgs& a, hipStream_t s)
{
  const uint32_t n = a.seq ? a.nhyp : a.njobs * a.nhyp;
  hipLaunchKernelGGL(sync_scan, dim3((n + 63) / 64), dim3(64), 0, s, a);
  return hipGetLastError();
}

hipError_t sync_launch_sss(const SyncArgs& a, hipStream_t s)
{
  hipLaunchKernelGGL(sync_sss, dim3(a.nhyp, a.njobs), dim3(64), (size_t)a.fft * sizeof(float2), s, a);
  return hipGetLastError();
}

hipError_t sync_launch_clear(float* p, size_t n, SyncState* st, uint32_t nhyp, uint32_t cp, hipStream_t s)
{
  hipLaunchKernelGGL(sync_clear, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, p, n, st, nhyp, cp);
  return hipGetLastError();
}

} // namespace mi355
