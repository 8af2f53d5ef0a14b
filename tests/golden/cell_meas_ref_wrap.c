/* tests/golden/cell_meas_ref_wrap.c -- glue for tests/golden/make_golden_cell_meas.py: drives the reference's
 * srslte_refsignal_dl_sync_t (compiled from the reference tree by that script) and supplies the srslte_dft_* functions
 * its sources call.  FFTW is not available where the fixture is recorded, so the transform below is a plain
 * double-precision DFT in this project's own words that honours the plans' mirror / dc / norm flags and the batched
 * ("guru") plans of the OFDM modulator: the reference's FFT is therefore a stand-in here and the recorded values carry
 * its rounding (one rounding to float per output) instead of an fp32 FFT's.
 *
 * The reference's refsignal_dl_sync.c is compiled as part of this translation unit (included from where it lies), so
 * that its static helpers can be called for the per-subframe records, and with its INFO trace routed to cmwrap_info,
 * which keeps the numbers the reference prints and does not return: peak, rms_avg and the stage-1 index of find_peak,
 * false_count of stage 3. */
#include <math.h>
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>

#include "srslte/phy/dft/dft.h"
#include "srslte/phy/sync/pss.h"
#include "srslte/phy/sync/sss.h"
#include "srslte/phy/utils/debug.h"

static void cmwrap_info(const char* fmt, ...);
#undef INFO
#define INFO(...) cmwrap_info(__VA_ARGS__)
#include "src/phy/sync/refsignal_dl_sync.c"

/* ---------------------------------------------------------------- the DFT stand-in */

typedef struct {
  double* cs; /* cos / sin of 2 pi m / n, m < n */
  cf_t *  gin, *gout;
  int     how_many, idist, odist;
} dft_tw_t;

int srslte_dft_plan_c(srslte_dft_plan_t* plan, int n, srslte_dft_dir_t dir)
{
  memset(plan, 0, sizeof(*plan));
  dft_tw_t* tw = calloc(1, sizeof(dft_tw_t));
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

int srslte_dft_plan_guru_c(srslte_dft_plan_t* plan, int n, srslte_dft_dir_t dir, cf_t* in, cf_t* out, int istride,
                           int ostride, int how_many, int idist, int odist)
{
  if (istride != 1 || ostride != 1 || srslte_dft_plan_c(plan, n, dir)) return -1;
  dft_tw_t* tw  = plan->p;
  tw->gin       = in;
  tw->gout      = out;
  tw->how_many  = how_many;
  tw->idist     = idist;
  tw->odist     = odist;
  plan->is_guru = true;
  return 0;
}

void srslte_dft_plan_free(srslte_dft_plan_t* plan)
{
  if (plan && plan->p) {
    free(((dft_tw_t*)plan->p)->cs);
    free(plan->p);
    plan->p    = NULL;
    plan->size = 0;
  }
}

int srslte_dft_replan(srslte_dft_plan_t* plan, const int n)
{
  const bool             mirror = plan->mirror, dc = plan->dc, norm = plan->norm;
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

/* out[k] = sum_m in[m] exp(-+ 2 pi i k m / n), accumulated in double, rounded once */
static void dft_plain(const srslte_dft_plan_t* plan, const double* xr, const double* xi, double scale, cf_t* y)
{
  const int     n   = plan->size;
  const double* cs  = ((dft_tw_t*)plan->p)->cs;
  const double  sgn = plan->forward ? -1.0 : 1.0;
  for (int k = 0; k < n; k++) {
    double ar = 0, ai = 0;
    for (int m = 0, idx = 0; m < n; m++) {
      const double c = cs[2 * idx], s = sgn * cs[2 * idx + 1];
      ar += xr[m] * c - xi[m] * s;
      ai += xr[m] * s + xi[m] * c;
      idx += k;
      if (idx >= n) idx -= n;
    }
    y[k] = (float)(ar * scale) + _Complex_I * (float)(ai * scale);
  }
}

/* Bin k of the transform sits at position pos(k) of a mirrored buffer: negative frequencies first, then the positive
 * ones, with the DC bin left out when dc is set.  Inputs of a backward transform are read through that map, outputs of
 * a forward transform are written through it. */
void srslte_dft_run_c(srslte_dft_plan_t* plan, const cf_t* in, cf_t* out)
{
  const int n = plan->size, half = n / 2, off = plan->dc ? 1 : 0;
  double*   xr = malloc(sizeof(double) * 2 * (size_t)n);
  double*   xi = xr + n;
  cf_t*     y  = malloc(sizeof(cf_t) * (size_t)n);
  for (int k = 0; k < n; k++) {
    cf_t v = 0;
    if (plan->mirror && !plan->forward) {
      if (k >= n - half) v = in[k - (n - half)];
      else if (k >= off) v = in[half + k - off];
    } else {
      v = in[k];
    }
    xr[k] = crealf(v), xi[k] = cimagf(v);
  }
  dft_plain(plan, xr, xi, plan->norm ? 1.0 / sqrtf((float)n) : 1.0, y);
  for (int k = 0; k < n; k++) {
    if (plan->mirror && plan->forward) {
      const int hl = (n + 1) / 2;
      if (k >= hl) out[k - hl] = y[k];
      else if (k >= off) out[(n - hl) + k - off] = y[k];
    } else {
      out[k] = y[k];
    }
  }
  free(xr);
  free(y);
}

void srslte_dft_run_c_zerocopy(srslte_dft_plan_t* plan, const cf_t* in, cf_t* out) { srslte_dft_run_c(plan, in, out); }

/* how_many plain transforms between the buffers the plan was made for */
void srslte_dft_run_guru_c(srslte_dft_plan_t* plan)
{
  const dft_tw_t* tw = plan->p;
  const int       n  = plan->size;
  double*         xr = malloc(sizeof(double) * 2 * (size_t)n);
  double*         xi = xr + n;
  for (int h = 0; h < tw->how_many; h++) {
    const cf_t* in = tw->gin + (size_t)h * tw->idist;
    for (int k = 0; k < n; k++) xr[k] = crealf(in[k]), xi[k] = cimagf(in[k]);
    dft_plain(plan, xr, xi, 1.0, tw->gout + (size_t)h * tw->odist);
  }
  free(xr);
}

/* ---------------------------------------------------------------- the driver */

static struct {
  int    peak_seen, stage3_seen;
  int    imax;
  double peak, rms;
  unsigned false_count;
} g_info;

static void cmwrap_info(const char* fmt, ...)
{
  va_list ap;
  va_start(ap, fmt);
  if (!strncmp(fmt, "pci=", 4)) { /* find_peak: pci, sf_len, imax, peak, rms, peak / rms */
    (void)va_arg(ap, unsigned);
    (void)va_arg(ap, unsigned);
    g_info.imax      = va_arg(ap, int);
    g_info.peak      = va_arg(ap, double);
    g_info.rms       = va_arg(ap, double);
    g_info.peak_seen = 1;
  } else if (!strncmp(fmt, "-- pci=", 7)) { /* stage 3: pci, ten floats, false_count */
    (void)va_arg(ap, unsigned);
    for (int i = 0; i < 10; i++) (void)va_arg(ap, double);
    g_info.false_count = va_arg(ap, unsigned);
    g_info.stage3_seen = 1;
  }
  va_end(ap);
}

void* cmwrap_create(void)
{
  srslte_refsignal_dl_sync_t* q = calloc(1, sizeof(*q));
  if (srslte_refsignal_dl_sync_init(q)) return NULL;
  return q;
}

int cmwrap_set_cell(void* h, uint32_t id, uint32_t nof_prb, uint32_t nof_ports)
{
  srslte_cell_t cell = {};
  cell.id            = id;
  cell.nof_prb       = nof_prb;
  cell.nof_ports     = nof_ports;
  cell.cp            = SRSLTE_CP_NORM;
  cell.frame_type    = SRSLTE_FDD;
  return srslte_refsignal_dl_sync_set_cell(h, cell);
}

uint32_t cmwrap_sf_len(void* h) { return ((srslte_refsignal_dl_sync_t*)h)->ifft.sf_sz; }

void cmwrap_sequence(void* h, uint32_t sf_idx, float* out)
{
  srslte_refsignal_dl_sync_t* q = h;
  memcpy(out, q->sequences[sf_idx], sizeof(cf_t) * q->ifft.sf_sz);
}

void cmwrap_free(void* h)
{
  srslte_refsignal_dl_sync_free(h);
  free(h);
}

void cmwrap_measure_sf(void* h, float* iq, uint32_t sf_idx, float* out3)
{
  srslte_refsignal_dl_sync_measure_sf(h, (cf_t*)iq, sf_idx, &out3[0], &out3[1], &out3[2]);
}

/* One srslte_refsignal_dl_sync_run.  iv: found, peak_index, stage1_peak, stage1_found, peak_shifted, sf_count,
 * false_count, false_alarm; fv: rsrp_dBfs, rssi_dBfs, rsrq_dB, cfo_Hz, peak_value, rms_avg.  sf: per measured subframe
 * (at most max_sf) sf_idx, rsrp, rssi, cfo, sss_strength, sss_strength_false, rsrp_false -- srslte_..._measure_sf and
 * refsignal_dl_pss_sss_strength called again over the subframes run went through. */
void cmwrap_run(void* h, float* iq, uint32_t nsamples, uint32_t max_sf, uint32_t* iv, float* fv, float* sf)
{
  srslte_refsignal_dl_sync_t* q = h;
  cf_t*                       buffer = (cf_t*)iq;
  memset(&g_info, 0, sizeof(g_info));
  srslte_refsignal_dl_sync_run(q, buffer, nsamples);
  iv[0] = q->found, iv[1] = q->peak_index;
  fv[0] = q->rsrp_dBfs, fv[1] = q->rssi_dBfs, fv[2] = q->rsrq_dB, fv[3] = q->cfo_Hz;
  fv[4] = (float)g_info.peak, fv[5] = (float)g_info.rms;
  const unsigned false_count = g_info.false_count;
  const int      stage3      = g_info.stage3_seen;
  const int      peak_idx    = srslte_refsignal_dl_sync_find_peak(q, buffer, nsamples);
  iv[2] = (uint32_t)g_info.imax;
  iv[3] = peak_idx >= 0;
  iv[4] = peak_idx >= 0 && peak_idx != g_info.imax;
  iv[5] = iv[6] = iv[7] = 0;
  if (peak_idx < 0) return;
  const uint32_t sf_len = q->ifft.sf_sz;
  uint32_t       count  = 0;
  for (uint32_t sf_idx = (20 - peak_idx / sf_len) % 10, n = peak_idx % sf_len; n < nsamples - sf_len + 1 && count < max_sf;
       sf_idx = (sf_idx + 1) % 10, n += sf_len, count++) {
    float* o = sf + 7 * count;
    memset(o, 0, 7 * sizeof(float));
    o[0] = (float)sf_idx;
    srslte_refsignal_dl_sync_measure_sf(q, &buffer[n], sf_idx, &o[1], &o[2], &o[3]);
    if (sf_idx % 5 == 0) {
      refsignal_dl_pss_sss_strength(q, &buffer[n], sf_idx, NULL, &o[4], &o[5]);
      srslte_refsignal_dl_sync_measure_sf(q, &buffer[n], sf_idx + 1, &o[6], NULL, NULL);
    }
  }
  iv[5] = count;
  iv[6] = stage3 ? false_count : 0;
  iv[7] = !q->found;
}
