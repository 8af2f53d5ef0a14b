/* tests/golden/sync_ref_wrap.c -- glue for tests/golden/make_golden_sync.py: drives the reference's srslte_sync_t
 * (compiled from the reference tree by that script) and supplies the srslte_dft_* functions the reference's sync
 * sources call.  FFTW is not available where the fixture is recorded, so the transform below is a plain
 * double-precision DFT in this project's own words that honours the plans' mirror / dc / norm flags: the reference's
 * FFT is therefore a stand-in here and the recorded values carry its rounding (one rounding to float per output)
 * instead of an fp32 FFT's. */
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "srslte/phy/dft/dft.h"
#include "srslte/phy/sync/sync.h"

/* ---------------------------------------------------------------- the DFT stand-in */

typedef struct {
  double* cs; /* cos / sin of 2 pi m / n, m < n */
} dft_tw_t;

int srslte_dft_plan_c(srslte_dft_plan_t* plan, int n, srslte_dft_dir_t dir)
{
  memset(plan, 0, sizeof(*plan));
  dft_tw_t* tw = malloc(sizeof(dft_tw_t));
  tw->cs       = malloc(sizeof(double) * 2 * (size_t)n);
  for (int m = 0; m < n; m++) {
    tw->cs[2 * m]     = cos(2.0 * M_PI * m / n);
    tw->cs[2 * m + 1] = sin(2.0 * M_PI * m / n);
  }
  plan->p         = tw;
  plan->init_size = n;
  plan->size      = n;
  plan->dir       = dir;
  plan->forward   = dir == SRSLTE_DFT_FORWARD;
  plan->mode      = SRSLTE_DFT_COMPLEX;
  return 0;
}

int srslte_dft_plan(srslte_dft_plan_t* plan, int n, srslte_dft_dir_t dir, srslte_dft_mode_t mode)
{
  return mode == SRSLTE_DFT_COMPLEX ? srslte_dft_plan_c(plan, n, dir) : -1;
}

void srslte_dft_plan_free(srslte_dft_plan_t* plan)
{
  if (plan && plan->p) {
    free(((dft_tw_t*)plan->p)->cs);
    free(plan->p);
    plan->p = NULL;
  }
}

int srslte_dft_replan(srslte_dft_plan_t* plan, const int n)
{
  const bool mirror = plan->mirror, dc = plan->dc, norm = plan->norm;
  const srslte_dft_dir_t dir = plan->dir;
  srslte_dft_plan_free(plan);
  srslte_dft_plan_c(plan, n, dir);
  plan->mirror = mirror, plan->dc = dc, plan->norm = norm;
  return 0;
}

void srslte_dft_plan_set_mirror(srslte_dft_plan_t* plan, bool v) { plan->mirror = v; }
void srslte_dft_plan_set_dc(srslte_dft_plan_t* plan, bool v) { plan->dc = v; }
void srslte_dft_plan_set_norm(srslte_dft_plan_t* plan, bool v) { plan->norm = v; }
void srslte_dft_plan_set_db(srslte_dft_plan_t* plan, bool v) { plan->db = v; }

/* Bin k of the transform sits at position pos(k) of a mirrored buffer: negative frequencies first, then the positive
 * ones, with the DC bin left out when dc is set.  Inputs of a backward transform are read through that map (the DC bin
 * is zero), outputs of a forward transform are written through it (the DC bin is dropped; the last position of the
 * buffer is then not written, as in the reference). */
void srslte_dft_run_c(srslte_dft_plan_t* plan, const cf_t* in, cf_t* out)
{
  const int     n   = plan->size, half = n / 2, off = plan->dc ? 1 : 0;
  const double* cs  = ((dft_tw_t*)plan->p)->cs;
  const double  sgn = plan->forward ? -1.0 : 1.0;
  double*       xr  = malloc(sizeof(double) * 2 * (size_t)n);
  double*       xi  = xr + n;
  for (int k = 0; k < n; k++) {
    cf_t v = 0;
    if (plan->mirror && !plan->forward) {
      if (k >= n - half) v = in[k - (n - half)];             /* negative frequencies: the buffer's first half */
      else if (k >= off) v = in[half + k - off];             /* positive ones, from DC (or 1) on */
    } else {
      v = in[k];
    }
    xr[k] = crealf(v), xi[k] = cimagf(v);
  }
  const double scale = plan->norm ? 1.0 / sqrtf((float)n) : 1.0;
  for (int k = 0; k < n; k++) {
    double ar = 0, ai = 0;
    for (int m = 0, idx = 0; m < n; m++) {
      const double c = cs[2 * idx], s = sgn * cs[2 * idx + 1];
      ar += xr[m] * c - xi[m] * s;
      ai += xr[m] * s + xi[m] * c;
      idx += k;
      if (idx >= n) idx -= n;
    }
    const cf_t y = (float)(ar * scale) + _Complex_I * (float)(ai * scale);
    if (plan->mirror && plan->forward) {
      const int hl = (n + 1) / 2;
      if (k >= hl) out[k - hl] = y;
      else if (k >= off) out[(n - hl) + k - off] = y;
    } else {
      out[k] = y;
    }
  }
  free(xr);
}

/* ---------------------------------------------------------------- the driver */

typedef struct {
  srslte_sync_t q;
} syncwrap_t;

void* syncwrap_create(uint32_t fft, uint32_t max_offset, uint32_t n_id_2, float threshold, float ema_alpha,
                      float cfo_ema_alpha, int cfo_pss, int pss_filt, int sss_en, int sss_alg, int detect_cp, int cp,
                      int detect_ft, int ft, float sss_thr)
{
  syncwrap_t* w = calloc(1, sizeof(*w));
  if (srslte_sync_init(&w->q, max_offset + fft, max_offset, fft)) return NULL;
  srslte_sync_set_N_id_2(&w->q, n_id_2);
  srslte_sync_set_threshold(&w->q, threshold);
  srslte_sync_set_em_alpha(&w->q, ema_alpha);
  srslte_sync_set_cfo_ema_alpha(&w->q, cfo_ema_alpha);
  srslte_sync_set_cfo_i_enable(&w->q, false);
  srslte_sync_set_cfo_cp_enable(&w->q, false, 0);
  srslte_sync_set_cfo_pss_enable(&w->q, cfo_pss != 0);
  srslte_sync_set_pss_filt_enable(&w->q, pss_filt != 0);
  srslte_sync_set_sss_eq_enable(&w->q, false);
  srslte_sync_sss_en(&w->q, sss_en != 0);
  /* this project's numbering (0 FULL, 1 PARTIAL_3, 2 DIFF) to the reference's enumerators */
  srslte_sync_set_sss_algorithm(&w->q, sss_alg == 0 ? SSS_FULL : sss_alg == 1 ? SSS_PARTIAL_3 : SSS_DIFF);
  srslte_sync_cp_en(&w->q, detect_cp != 0);
  srslte_sync_set_cp(&w->q, (srslte_cp_t)cp);
  w->q.frame_type        = (srslte_frame_type_t)ft;
  w->q.detect_frame_type = detect_ft != 0;
  srslte_sss_set_threshold(&w->q.sss, sss_thr);
  return w;
}

void syncwrap_reset(void* h)
{
  syncwrap_t* w = h;
  srslte_sync_reset(&w->q);
  srslte_sync_cfo_reset(&w->q, 0);
}

void syncwrap_free(void* h)
{
  syncwrap_t* w = h;
  srslte_sync_free(&w->q);
  free(w);
}

/* srslte_pss_generate / srslte_sss_generate, for the fixture's sequences */
int syncwrap_pss_generate(uint32_t n_id_2, float* pss62) { return srslte_pss_generate((cf_t*)pss62, n_id_2); }
void syncwrap_sss_generate(uint32_t cell_id, float* sf0, float* sf5) { srslte_sss_generate(sf0, sf5, cell_id); }

/* one srslte_sync_find; iv: ret, peak_pos, sss_available, sss_detected, m0, m1, n_id_1, sf_idx, cell_id, cp,
 * frame_type; fv: peak_value, peak_abs, cfo_pss, cfo_pss_mean, m0_value, m1_value, sss_corr, M_norm_avg, M_ext_avg */
int syncwrap_find(void* h, const float* iq, uint32_t find_offset, int32_t* iv, float* fv)
{
  syncwrap_t* w   = h;
  uint32_t    pos = 0;
  const int   ret = srslte_sync_find(&w->q, (const cf_t*)iq, find_offset, &pos);
  iv[0]  = ret;
  iv[1]  = (int32_t)pos;
  iv[2]  = srslte_sync_sss_available(&w->q);
  iv[3]  = srslte_sync_sss_detected(&w->q);
  iv[4]  = (int32_t)w->q.m0;
  iv[5]  = (int32_t)w->q.m1;
  iv[6]  = (int32_t)w->q.N_id_1;
  iv[7]  = (int32_t)w->q.sf_idx;
  iv[8]  = srslte_sync_get_cell_id(&w->q);
  iv[9]  = (int32_t)w->q.cp;
  iv[10] = (int32_t)w->q.frame_type;
  fv[0]  = srslte_sync_get_peak_value(&w->q);
  fv[1]  = w->q.pss.peak_value;
  fv[2]  = w->q.cfo_pss;
  fv[3]  = w->q.cfo_pss_mean;
  fv[4]  = w->q.m0_value;
  fv[5]  = w->q.m1_value;
  fv[6]  = srslte_sync_sss_correlation_peak(&w->q);
  fv[7]  = w->q.M_norm_avg;
  fv[8]  = w->q.M_ext_avg;
  return ret;
}
