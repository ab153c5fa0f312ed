// knn_api.cpp -- C ABI (include/knn_amd.h) over the gfx950 kernels.
//
// One knn_ctx per GPU (≙ one MPI rank of the reference, cpp:121-125).  The
// train set lives in HBM in two forms: the caller's fp64 rows (exact
// re-rank, ≙ Data_train cpp:140) and a padded fp32 copy + per-row seeds for
// the MFMA candidate pass.  Queries are classified by the pipeline in
// knn_cand.hip / knn_select.hip; there is no host compute path.
#include <hip/hip_runtime.h>

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "../../include/knn_amd.h"
#include "knn_api_internal.h"
#include "knn_csv_num.h"
#include "knn_kernels.h"

using namespace knnk;

namespace {
thread_local std::string g_err;
}

void knn_set_error(const char* fmt, const char* a, long long b) {
  char buf[512];
  snprintf(buf, sizeof buf, fmt, a, b);
  g_err = buf;
}

int knn_fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

#define HIP_TRY(expr)                                                                   \
  do {                                                                                  \
    hipError_t e_ = (expr);                                                             \
    if (e_ != hipSuccess)                                                               \
      return knn_fail(KNN_ERR_DEVICE, std::string(#expr " failed: ") + hipGetErrorString(e_)); \
  } while (0)

int DevBuf::ensure(size_t bytes) {
  if (cap >= bytes && p) return KNN_OK;
  if (p) (void)hipFree(p);
  p = nullptr;
  cap = 0;
  if (bytes == 0) bytes = 16;
  if (hipMalloc(&p, bytes) != hipSuccess) {
    p = nullptr;
    return knn_fail(KNN_ERR_NOMEM, "hipMalloc of " + std::to_string(bytes) + " bytes failed");
  }
  cap = bytes;
  return KNN_OK;
}
void DevBuf::release() {
  if (p) (void)hipFree(p);
  p = nullptr;
  cap = 0;
}

static int device_guard(knn_ctx* ctx) {
  if (!ctx) return knn_fail(KNN_ERR_ARG, "null context");
  HIP_TRY(hipSetDevice(ctx->device));
  return KNN_OK;
}

// the stream a *_device call runs on: the caller's, or the context's own
static hipStream_t stream_of(const knn_ctx* ctx, void* stream) {
  return stream ? (hipStream_t)stream : ctx->stream;
}

// a host-API output: bytes from the staging buffer to dst where the caller
// asked for it (dst nullable) and there is something to copy
static int copy_back(void* dst, const void* src, size_t bytes, hipStream_t s) {
  if (dst && bytes) HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s));
  return KNN_OK;
}

// Drops the folds of knn_set_folds: the sub-contexts and the fold-major copy
// (they belong to one train set, like the group ids).
static void fold_clear(knn_ctx* ctx) {
  for (knn_ctx* sub : ctx->fold_ctx) knn_destroy(sub);
  ctx->fold_ctx.clear();
  ctx->fold_off.clear();
  ctx->fold_rows.clear();
  ctx->n_folds = ctx->fold_max = 0;
  ctx->fold_X.release();
  ctx->fold_lab.release();
}

extern "C" {

const char* knn_version(void) { return "mpi-knn-amd 0.1 (gfx950)"; }
const char* knn_last_error(void) { return g_err.c_str(); }

int knn_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int knn_create(knn_ctx** out, int device) {
  if (!out) return knn_fail(KNN_ERR_ARG, "null out pointer");
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
    return knn_fail(KNN_ERR_DEVICE, "no HIP device available (the KNN path has no CPU fallback)");
  if (device < 0 || device >= n) return knn_fail(KNN_ERR_ARG, "device index out of range");
  HIP_TRY(hipSetDevice(device));
  knn_ctx* c = new knn_ctx();
  c->device = device;
  // a blocking stream: ordered after work the caller queued on the legacy
  // default stream (e.g. torch producing the device inputs), so device
  // pointers handed to *_device calls with stream = NULL are safe to read
  if (hipStreamCreateWithFlags(&c->stream, hipStreamDefault) != hipSuccess) {
    delete c;
    return knn_fail(KNN_ERR_DEVICE, "hipStreamCreate failed");
  }
  // per-call rescan counts, written by the device (host-mapped pinned memory)
  if (hipHostMalloc((void**)&c->h_counts, sizeof(int) * 4, hipHostMallocMapped) != hipSuccess ||
      hipHostGetDevicePointer((void**)&c->d_counts, c->h_counts, 0) != hipSuccess ||
      hipEventCreateWithFlags(&c->done_ev, hipEventDisableTiming) != hipSuccess ||
      c->totals.ensure(3 * sizeof(unsigned long long)) != KNN_OK ||
      hipMemset(c->totals.p, 0, 3 * sizeof(unsigned long long)) != hipSuccess) {
    knn_destroy(c);
    return knn_fail(KNN_ERR_DEVICE, "context setup (pinned counters / events) failed");
  }
  c->h_counts[0] = c->h_counts[1] = 0;
  if (hipDeviceGetAttribute(&c->cu_count, hipDeviceAttributeMultiprocessorCount, device) !=
          hipSuccess ||
      c->cu_count <= 0)
    c->cu_count = 256;
  if (const char* e = getenv("KNN_PRECISION")) {
    if (!strcmp(e, "fp32")) c->precision = KNN_PRECISION_FP32;
    else if (!strcmp(e, "bf16x3")) c->precision = KNN_PRECISION_BF16X3;
    else if (!strcmp(e, "fp16")) c->precision = KNN_PRECISION_FP16;
  }
  *out = c;
  return KNN_OK;
}

int knn_destroy(knn_ctx* ctx) {
  if (!ctx) return KNN_OK;
  (void)hipSetDevice(ctx->device);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  fold_clear(ctx);
  for (DevBuf* b : ctx->all_bufs()) b->release();
  for (auto& tc : ctx->ring)
    for (auto& e : tc.ev)
      if (e) (void)hipEventDestroy(e);
  if (ctx->done_ev) (void)hipEventDestroy(ctx->done_ev);
  if (ctx->h_counts) (void)hipHostFree(ctx->h_counts);
  if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
  delete ctx;
  return KNN_OK;
}

}  // extern "C"

// Integer-coded train sets (knn_prep.hip, int8 images): every value x =
// (c_i + k) / 2^s with an integer code k in [-128, 127] per dimension -- the
// 8-bit grid of SIFT-like byte features, or of the reference's CSVs of
// k/256 values.  s = the largest number of fractional bits of any value; the
// centre c_i is the middle of dimension i's code range.  Sets ctx->i8_ok.
static int detect_i8(knn_ctx* ctx, const double* dX, int64_t n, int d) {
  ctx->i8_ok = false;
  // (d <= 256: the int8 passes; up to 1024: the wide L1 pass, "i8l1" = 2)
  if (pad_dim_i8(d) <= 0 && pad_dim_i8l1w(d) <= 0) return KNN_OK;
  int rc;
  if ((rc = ctx->i8_gs.ensure((size_t)(col_mean_blocks(n) * 2 + 2) * d * sizeof(double) + 16)))
    return rc;
  double* part = (double*)ctx->i8_gs.p;
  double* out = part + (size_t)col_mean_blocks(n) * 2 * d;
  unsigned* frac = (unsigned*)(out + 2 * d);
  HIP_TRY(hipMemsetAsync(frac, 0, sizeof(unsigned), ctx->stream));
  launch_grid_stats(dX, n, d, part, out, frac, ctx->stream);
  HIP_TRY(hipGetLastError());
  std::string buf((size_t)2 * d * sizeof(double) + sizeof(unsigned), '\0');
  HIP_TRY(hipMemcpyAsync(&buf[0], out, buf.size(), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  const double* lohi = (const double*)buf.data();
  unsigned s;
  memcpy(&s, buf.data() + 2 * d * sizeof(double), sizeof s);
  if (s > 30) return KNN_OK;
  std::string cent((size_t)2 * d * sizeof(double), '\0');
  double* c = (double*)&cent[0];
  for (int i = 0; i < d; ++i) {
    const double lo = std::ldexp(lohi[i], (int)s), hi = std::ldexp(lohi[d + i], (int)s);
    if (!(hi - lo <= 255.0) || !(std::fabs(lo) < 0x1p50) || !(std::fabs(hi) < 0x1p50)) return KNN_OK;
    c[i] = std::floor((lo + hi + 1.0) / 2.0);        // codes x 2^s - c in [-128, 127]
    c[d + i] = std::ldexp(c[i], -(int)s);            // the same centre in value units
  }
  if ((rc = ctx->i8_cent.ensure((size_t)2 * d * sizeof(double)))) return rc;
  HIP_TRY(hipMemcpy(ctx->i8_cent.p, c, (size_t)2 * d * sizeof(double), hipMemcpyHostToDevice));
  ctx->i8_s = (int)s;
  ctx->i8_ok = true;
  return KNN_OK;
}

// k-means on a strided sample (8 Lloyd rounds), every row assigned, rows
// counting-sorted by the chain rank of their region (knn_order.hip).
static int build_order(knn_ctx* ctx, const double* dX, const double* mu, int64_t n, int d, int jx,
                       int P) {
  const int64_t ns = std::min<int64_t>(n, 65536);
  const int64_t stride = n / ns;
  const int64_t nb = region_sort_blocks(n);
  int rc;
  if ((rc = ctx->ord_cent.ensure((size_t)kRegionMax * d * sizeof(float)))) return rc;
  if ((rc = ctx->ord_cnorm.ensure(kRegionMax * sizeof(float)))) return rc;
  if ((rc = ctx->ord_img.ensure(kRegionImgBytes))) return rc;
  if ((rc = ctx->ord_rank.ensure(kRegionMax * sizeof(int)))) return rc;
  if ((rc = ctx->ord_rstart.ensure(kRegionMax * sizeof(int)))) return rc;
  if ((rc = ctx->ord_tot.ensure(kRegionMax * sizeof(int)))) return rc;
  if ((rc = ctx->ord_key.ensure((size_t)n * sizeof(int)))) return rc;
  if ((rc = ctx->ord_bcnt.ensure((size_t)nb * kRegionMax * sizeof(int)))) return rc;
  if ((rc = ctx->ord_perm.ensure((size_t)n * sizeof(int)))) return rc;
  if ((rc = ctx->ord_ipos.ensure((size_t)n * sizeof(int)))) return rc;
  float* cent = (float*)ctx->ord_cent.p;
  int* rank = (int*)ctx->ord_rank.p;
  int* key = (int*)ctx->ord_key.p;
  launch_region_kmeans(dX, mu, ns, d, stride, jx, P, 8, cent, (unsigned short*)ctx->ord_img.p,
                       (float*)ctx->ord_cnorm.p, key, rank, ctx->stream);
  launch_region_assign(dX, mu, n, d, 1, jx, (const unsigned short*)ctx->ord_img.p,
                       (const float*)ctx->ord_cnorm.p, rank, key, nullptr, ctx->stream);
  ctx->ord_bcnt_zero = 0;  // (the train sort leaves its prefix sums there)
  launch_region_sort(key, n, (int*)ctx->ord_bcnt.p, (int*)ctx->ord_tot.p, (int*)ctx->ord_perm.p,
                     (int*)ctx->ord_ipos.p, nullptr, nullptr, (int*)ctx->ord_rstart.p, ctx->stream);
  HIP_TRY(hipGetLastError());
  ctx->ord_P = P;
  return KNN_OK;
}

// The windows sorted by the int8 code norm (the seeds' own; ||x - mu||^2 for
// other sets), on top of the region order when it is on.
static int build_norm_blocks(knn_ctx* ctx, const double* dX, int64_t n, int d) {
  int rc;
  if ((rc = ctx->ord_key.ensure((size_t)n * sizeof(int)))) return rc;
  if ((rc = ctx->ord_perm.ensure((size_t)n * sizeof(int)))) return rc;
  if ((rc = ctx->ord_ipos.ensure((size_t)n * sizeof(int)))) return rc;
  const int* perm0 = nullptr;
  if (ctx->ord_P) {
    if ((rc = ctx->ord_perm0.ensure((size_t)n * sizeof(int)))) return rc;
    HIP_TRY(hipMemcpyAsync(ctx->ord_perm0.p, ctx->ord_perm.p, (size_t)n * sizeof(int),
                           hipMemcpyDeviceToDevice, ctx->stream));
    perm0 = (const int*)ctx->ord_perm0.p;
  }
  const bool i8 = ctx->i8_ok;
  // norm ranks interleaved over the int8 kernel's lane lists and sub-tiles
  // spread over the window's tiles (nblk 2: the plain sorted windows, round
  // 5's layout; 3: the interleave only)
  const int il = !i8 || ctx->tune.nblk == 2 ? 0
                 : i8_kernel_d(ctx->tune, d) | (ctx->tune.nblk == 3 ? 0 : 16);
  launch_norm_blocks(dX, i8 ? (const double*)ctx->i8_cent.p : nullptr, ctx->i8_s,
                     (const double*)ctx->mu.p, n, d, perm0, (uint32_t*)ctx->ord_key.p,
                     (int*)ctx->ord_perm.p, (int*)ctx->ord_ipos.p, il, ctx->stream);
  HIP_TRY(hipGetLastError());
  ctx->ord_nb = true;
  return KNN_OK;
}

// Builds the fp32 candidate copy + seeds + norm stats from fp64 rows that
// already sit on the device.
static int build_train(knn_ctx* ctx, const double* dX, const int32_t* dlab, int64_t n, int d,
                       int class_cnt, int64_t idx_off) {
  const int DP = pad_dim(d);
  if (!cand_supported(DP))
    return knn_fail(KNN_ERR_ARG, "dimension " + std::to_string(d) + " not supported by this build");
  const int64_t n_pad = (n + kRowAlign - 1) / kRowAlign * kRowAlign;
  int rc;
  ctx->groups = nullptr;  // group ids belong to one train set (knn_set_groups)
  ctx->n_groups = ctx->gmax = 0;
  if (ctx->n_folds) {  // and so do the folds (knn_set_folds); their work may still run
    HIP_TRY(hipDeviceSynchronize());
    fold_clear(ctx);
  }
  // padded rows [payload | seeds] (+1 KiB slack: the last LDS-DMA piece of
  // the last tile may read past the final row)
  if ((rc = ctx->X32.ensure((size_t)n_pad * (DP + 4) * sizeof(float) + 1024))) return rc;
  if ((rc = ctx->xl2.ensure((size_t)n_pad * sizeof(float)))) return rc;
  if ((rc = ctx->xl1.ensure((size_t)n_pad * sizeof(float)))) return rc;
  if ((rc = ctx->stats.ensure(6 * sizeof(unsigned long long)))) return rc;
  if ((rc = ctx->mu.ensure((size_t)d * sizeof(double)))) return rc;
  if ((rc = ctx->mu_part.ensure((size_t)col_mean_blocks(n) * d * sizeof(double)))) return rc;
  launch_col_mean(dX, n, d, (double*)ctx->mu_part.p, (double*)ctx->mu.p, ctx->stream);
  HIP_TRY(hipMemsetAsync(ctx->stats.p, 0, 6 * sizeof(unsigned long long), ctx->stream));
  unsigned long long* st_d = (unsigned long long*)ctx->stats.p;
  // operand scale 2^jx: max |x_i - mu_i| * 2^jx in [2^8, 2^9) (knn_prep.hip);
  // with it, the count of non-finite values and of labels out of range
  launch_absmax(dX, (const double*)ctx->mu.p, n, d, st_d + 2, st_d + 4, ctx->stream);
  launch_label_check(dlab, n, class_cnt, st_d + 5, ctx->stream);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(ctx->h_stats + 2, st_d + 2, 4 * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  ctx->trained = false;
  if (ctx->h_stats[4])
    return knn_fail(KNN_ERR_ARG, "train set holds " + std::to_string(ctx->h_stats[4]) +
                                     " non-finite values (NaN / inf): distances undefined");
  if (ctx->h_stats[5])
    return knn_fail(KNN_ERR_ARG, std::to_string(ctx->h_stats[5]) +
                                     " train labels outside [0, class_cnt)");
  memcpy(&ctx->xamax, &ctx->h_stats[2], 8);
  if ((rc = detect_i8(ctx, dX, n, d))) return rc;
  int e = 0;
  if (ctx->xamax > 0.0) (void)std::frexp(ctx->xamax, &e);  // xamax < 2^e
  // |x - mu| up to 2^400 (beyond, fp32 operands could overflow); tiny data
  // is scaled up at most 2^450 (smaller values are covered by the bound's
  // absolute terms)
  if (!(ctx->xamax < std::ldexp(1.0, 400)))
    return knn_fail(KNN_ERR_ARG, "train values out of range (|x - mean| must be < 2^400 and finite)");
  const int jx = std::min(9 - e, 450);
  // centre on the 2^-(jx+2) grid: data on any coarser grid (bytes scaled by a
  // power of two, integers, ...) is then exact in the fp16 operands, whose
  // measured representation error vanishes from the bound;
  // the shift is <= 2^-11 of max |x - mu|, immaterial for the centring
  launch_round_mu((double*)ctx->mu.p, d, jx + 2, ctx->stream);
  ctx->ord_P = 0;
  ctx->ord_nb = false;
  ctx->ord_bcnt_zero = 0;
  const int P = region_count(ctx->tune, ctx->i8_ok, n, d);
  if (P > 0 && (rc = build_order(ctx, dX, (const double*)ctx->mu.p, n, d, jx, P))) return rc;
  if (norm_blocks_on(ctx->tune, ctx->i8_ok, n, d) && (rc = build_norm_blocks(ctx, dX, n, d))) return rc;
  const int* perm = ctx->ord_P || ctx->ord_nb ? (const int*)ctx->ord_perm.p : nullptr;
  launch_prep_train(dX, (const double*)ctx->mu.p, n, d, DP, n_pad, jx, (float*)ctx->X32.p,
                    (float*)ctx->xl2.p, (float*)ctx->xl1.p, st_d, ctx->stream, perm);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(ctx->h_stats, st_d, 2 * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  double x2, x1;
  memcpy(&x2, &ctx->h_stats[0], 8);
  memcpy(&x1, &ctx->h_stats[1], 8);
  TrainDev& t = ctx->train;
  t.X64 = dX;
  t.mu = (const double*)ctx->mu.p;
  t.lab = dlab;
  t.X32 = (const float*)ctx->X32.p;
  t.xinit_l2 = (const float*)ctx->xl2.p;
  t.xinit_l1 = (const float*)ctx->xl1.p;
  t.n = n;
  t.n_pad = n_pad;
  t.d = d;
  t.DP = DP;
  t.x2max = x2;
  t.x1max = x1;
  t.jx = jx;
  t.perm = perm;
  t.ipos = perm ? (const int*)ctx->ord_ipos.p : nullptr;
  ctx->class_cnt = class_cnt;
  ctx->idx_off = idx_off;
  ctx->DPb = 0;  // bf16x3 / fp16 copies are rebuilt lazily for the new train set
  ctx->DPh = 0;
  ctx->DPs = 0;
  ctx->DPi = 0;
  ctx->DPiw = 0;
  ctx->DPu = 0;
  ctx->DPuw = 0;
  ctx->smp_kind = 0;  // the seeding sample is rebuilt for the new train set
  ctx->i8_off = false;
  ctx->fp16_off = false;
  ctx->auto_pending = false;
  ctx->trained = true;
  return KNN_OK;
}

// The bf16 hi/lo copy of the train rows for the bf16x3 L2 candidate pass,
// built on first use (same row padding as X32).
static int ensure_bf16x3(knn_ctx* ctx, hipStream_t s) {
  const TrainDev& t = ctx->train;
  const int DPb = pad_dim_bf16x3(t.d);
  if (DPb <= 0) return knn_fail(KNN_ERR_ARG, "bf16x3 path supports d <= 256");
  if (ctx->DPb == DPb) return KNN_OK;
  int rc;
  if (bf16x3_streamed(DPb)) {
    // S3 stream kernel: tile-chunk images (4 B per dim: hi + lo) + seeds,
    // rows padded to whole 256-row tiles
    const int64_t n3 = (t.n + kS3Rows - 1) / kS3Rows * kS3Rows;
    if ((rc = ctx->XB.ensure((size_t)n3 * DPb * 4))) return rc;
    if ((rc = ctx->XS.ensure((size_t)n3 * sizeof(float)))) return rc;
    launch_prep_split_tiled(t.X64, t.mu, t.n, t.d, DPb, n3, std::ldexp(1.0, t.jx), (unsigned short*)ctx->XB.p, t.xinit_l2,
                            (float*)ctx->XS.p, s, t.perm);
  } else {
    if ((rc = ctx->XB.ensure((size_t)t.n_pad * (DPb + 4) * sizeof(float) + 1024))) return rc;
    launch_prep_split(t.X64, t.mu, t.n, t.d, DPb, t.n_pad, std::ldexp(1.0, t.jx), (unsigned short*)ctx->XB.p,
                      2 * (DPb + 4), t.xinit_l2, t.xinit_l1, s, t.perm);
  }
  HIP_TRY(hipGetLastError());
  ctx->DPb = DPb;
  return KNN_OK;
}

// TrainDev::dxmax of an fp16 image just built: the builder's running max of
// the rows' squared representation error (st_d), read back.
static int read_dxmax(knn_ctx* ctx, const unsigned long long* st_d, hipStream_t s) {
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(ctx->h_stats + 3, st_d, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  double dx2;
  memcpy(&dx2, &ctx->h_stats[3], 8);
  // + the fp64 rounding of x - mu itself (<= 2^-53 relative per element)
  ctx->train.dxmax = std::sqrt(dx2) * (1.0 + 1e-12) + 0x1p-50 * std::sqrt(ctx->train.x2max);
  return KNN_OK;
}

// The fp16 copy of the train rows for kernel metric 4:
// 2^jx (x - mu) in fp16 (the operand scale of every path) + the L2 seeds;
// same row count as X32, rows of DP/2 + 4 floats.
static int ensure_fp16(knn_ctx* ctx, hipStream_t s) {
  const TrainDev& t = ctx->train;
  const int DPh = pad_dim_fp16(t.d);
  if (DPh <= 0) return knn_fail(KNN_ERR_ARG, "fp16 path supports d <= 256");
  const int swz = ctx->tune.xhswz != 0;  // chunk swizzle of the image (xh_swz)
  if (ctx->DPh == DPh && ctx->xh_swz == swz) return KNN_OK;
  int rc;
  if ((rc = ctx->XH.ensure((size_t)t.n_pad * (DPh / 2 + 4) * sizeof(float) + 1024))) return rc;
  unsigned long long* st_d = (unsigned long long*)ctx->stats.p + 3;
  HIP_TRY(hipMemsetAsync(st_d, 0, 8, s));
  launch_prep_half_train(t.X64, t.mu, t.n, t.d, DPh, t.n_pad, t.jx,
                         (unsigned short*)ctx->XH.p, t.xinit_l2, st_d, swz, s, t.perm);
  if ((rc = read_dxmax(ctx, st_d, s))) return rc;
  ctx->DPh = DPh;
  ctx->xh_swz = swz;
  return KNN_OK;
}

// The int8 image for kernel metrics 5 / 6 / 7 (knn_prep.hip): codes x 2^s - c
// of every row (16-B chunks swizzled as the fp16 image for metric 5, plain for
// metric 6) + the accumulator seeds -ceil(||k||^2 / 2); rows of DP + 16
// bytes, n_pad rows.  Metric 7 (L1 on the codes) reads metric 6's image, its
// codes only; the fp32 image of set_train stays for the rescan's filter.
static int ensure_i8(knn_ctx* ctx, int kmetric, hipStream_t s) {
  const TrainDev& t = ctx->train;
  const int DPi = kmetric >= 6 ? pad_dim_i8w(t.d) : pad_dim_i8(t.d);
  const int swz = kmetric >= 6 ? 0 : 1;
  if (!ctx->i8_ok || DPi <= 0) return knn_fail(KNN_ERR_ARG, "train set not integer-coded (int8 pass)");
  if (ctx->DPi == DPi && ctx->i8_swz == swz) return KNN_OK;
  int rc;
  if ((rc = ctx->XI.ensure((size_t)t.n_pad * (DPi + 16) + 1024))) return rc;
  unsigned* cmax = (unsigned*)((unsigned long long*)ctx->stats.p + 3);
  HIP_TRY(hipMemsetAsync(cmax, 0, 8, s));
  launch_prep_i8_train(t.X64, (const double*)ctx->i8_cent.p, t.n, t.d, DPi, t.n_pad, ctx->i8_s,
                       (signed char*)ctx->XI.p, cmax, swz, s, t.perm);
  HIP_TRY(hipGetLastError());
  unsigned cm = 0;
  HIP_TRY(hipMemcpyAsync(&cm, cmax, sizeof cm, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  ctx->i8_x2max = std::ldexp((double)cm, -2 * ctx->i8_s);
  ctx->DPi = DPi;
  ctx->i8_swz = swz;
  return KNN_OK;
}

// The image of kernel metric 7 at 256 < d <= 1024 (knn_cand_sad_wide.hip):
// plain rows of DP code bytes in its own buffer, built on the first wide L1
// call; the d <= 256 images are untouched.
static int ensure_i8_wide(knn_ctx* ctx, hipStream_t s) {
  const TrainDev& t = ctx->train;
  const int DPw = pad_dim_i8l1w(t.d);
  if (!ctx->i8_ok || DPw <= 0)
    return knn_fail(KNN_ERR_ARG, "train set not integer-coded (wide L1 pass on int8 codes)");
  if (ctx->DPiw == DPw) return KNN_OK;
  int rc;
  if ((rc = ctx->XIW.ensure((size_t)t.n_pad * DPw + 1024))) return rc;
  launch_prep_i8_rows(t.X64, (const double*)ctx->i8_cent.p, t.n, t.d, DPw, t.n_pad, ctx->i8_s,
                      (signed char*)ctx->XIW.p, s, t.perm);
  HIP_TRY(hipGetLastError());
  ctx->DPiw = DPw;
  return KNN_OK;
}

// The image of kernel metric 8 (knn_cand_fix16.hip): rows of DP 16-bit
// fixed-point codes of 2^e (x - mu), e = jx + 5 -- max |x - mu| 2^jx < 2^9
// (build_train), so the train codes stay within 32768 +- 2^14, half the range,
// and jx's own cap keeps e defined for a constant train set -- in its own
// buffer, built on the first such call; with it the largest coding error of
// a row (u16_dx, code units), which the merge's bound adds.
static int ensure_u16(knn_ctx* ctx, hipStream_t s) {
  const TrainDev& t = ctx->train;
  const int DPu = pad_dim_u16l1(t.d);
  if (DPu <= 0) return knn_fail(KNN_ERR_ARG, "16-bit fixed-point L1 pass supports d <= 256");
  if (ctx->DPu == DPu) return KNN_OK;
  int rc;
  if ((rc = ctx->XU.ensure((size_t)t.n_pad * DPu * sizeof(unsigned short)))) return rc;
  const int e = t.jx + 5;
  unsigned long long* st_d = (unsigned long long*)ctx->stats.p + 3;
  HIP_TRY(hipMemsetAsync(st_d, 0, 8, s));
  launch_prep_u16_train(t.X64, t.mu, t.n, t.d, DPu, t.n_pad, e, (unsigned short*)ctx->XU.p, st_d, s,
                        t.perm);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(ctx->h_stats + 3, st_d, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  memcpy(&ctx->u16_dx, &ctx->h_stats[3], 8);
  ctx->u16_e = e;
  ctx->DPu = DPu;
  return KNN_OK;
}

// The image of kernel metric 8 at 256 < d <= 1024 (knn_cand_fix16_wide.hip):
// the same codes at the same scale as 32-row tiles of dim slabs, in its own
// buffer, built on the first such call (train order: no region order and no
// norm blocks above 256 dims); u16_dx is measured by the same row pass.
static int ensure_u16_wide(knn_ctx* ctx, hipStream_t s) {
  const TrainDev& t = ctx->train;
  const int DPw = pad_dim_u16l1w(t.d);
  if (DPw <= 0)
    return knn_fail(KNN_ERR_ARG, "wide 16-bit fixed-point L1 pass supports 256 < d <= 1024");
  if (ctx->DPuw == DPw) return KNN_OK;
  int rc;
  if ((rc = ctx->XUW.ensure((size_t)t.n_pad * DPw * sizeof(unsigned short)))) return rc;
  const int e = t.jx + 5;
  unsigned long long* st_d = (unsigned long long*)ctx->stats.p + 3;
  HIP_TRY(hipMemsetAsync(st_d, 0, 8, s));
  launch_prep_u16_train_wide(t.X64, t.mu, t.n, t.d, DPw, t.n_pad, e, (unsigned short*)ctx->XUW.p,
                             st_d, s, t.perm);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(ctx->h_stats + 3, st_d, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  memcpy(&ctx->u16_dx, &ctx->h_stats[3], 8);
  ctx->u16_e = e;
  ctx->DPuw = DPw;
  return KNN_OK;
}

// The fp16 S3 image (d > 256, cand_s3_kernel<R, true>): 2^jx (x - mu) in
// fp16 tile-chunk images + the L2 seeds; the representation error measured
// as for the resident copy.
static int ensure_fp16_s3(knn_ctx* ctx, hipStream_t s) {
  const TrainDev& t = ctx->train;
  const int DPs = pad_dim_fp16_s3(t.d);
  if (DPs <= 0) return knn_fail(KNN_ERR_ARG, "fp16 S3 path needs d > 256");
  if (ctx->DPs == DPs) return KNN_OK;
  int rc;
  const int64_t n3 = (t.n + kS3Rows - 1) / kS3Rows * kS3Rows;
  if ((rc = ctx->XT16.ensure((size_t)n3 * DPs * 2))) return rc;
  // (+1 KB: cand_qres_kernel stages a sub-tile's 32 seeds as one 1-KB piece)
  if ((rc = ctx->XS16.ensure((size_t)n3 * sizeof(float) + 1024))) return rc;
  unsigned long long* st_d = (unsigned long long*)ctx->stats.p + 3;
  HIP_TRY(hipMemsetAsync(st_d, 0, 8, s));
  launch_prep_half_tiled(t.X64, t.mu, t.n, t.d, DPs, n3, t.jx, 1.0, (unsigned short*)ctx->XT16.p,
                         t.xinit_l2, (float*)ctx->XS16.p, nullptr, st_d, s, t.perm);
  if ((rc = read_dxmax(ctx, st_d, s))) return rc;
  ctx->DPs = DPs;
  return KNN_OK;
}

static int ensure_sample(knn_ctx* ctx, int kmetric, int DP, int64_t ns, hipStream_t s) {
  const TrainDev& t = ctx->train;
  if (ctx->smp_kind == kmetric && ctx->smp_dp == DP && ctx->smp_n == ns &&
      (kmetric == 5 || ctx->smp_swz == ctx->xh_swz))
    return KNN_OK;
  const int d = t.d;
  const int64_t stride = t.n / ns;  // sample row i = train row i * stride
  const size_t row_bytes = kmetric == 5 ? (size_t)DP + 16 : (size_t)(DP / 2 + 4) * 4;
  int rc;
  if ((rc = ctx->smp_x64.ensure((size_t)ns * d * sizeof(double)))) return rc;
  if ((rc = ctx->smp_xl2.ensure((size_t)ns * sizeof(float)))) return rc;
  if ((rc = ctx->smp_img.ensure((size_t)ns * row_bytes + 1024))) return rc;
  if ((rc = ctx->smp_scr.ensure(16))) return rc;
  HIP_TRY(hipMemcpy2DAsync(ctx->smp_x64.p, (size_t)d * 8, t.X64, (size_t)stride * d * 8,
                           (size_t)d * 8, (size_t)ns, hipMemcpyDeviceToDevice, s));
  HIP_TRY(hipMemsetAsync(ctx->smp_scr.p, 0, 16, s));
  if (kmetric == 5) {
    launch_prep_i8_train((const double*)ctx->smp_x64.p, (const double*)ctx->i8_cent.p, ns, d, DP, ns,
                         ctx->i8_s, (signed char*)ctx->smp_img.p, (unsigned*)ctx->smp_scr.p, 1, s);
  } else {
    // the fp16 image's seeds are the rows' fl32 ||x'||^2 of the main copy
    HIP_TRY(hipMemcpy2DAsync(ctx->smp_xl2.p, 4, t.xinit_l2, (size_t)stride * 4, 4, (size_t)ns,
                             hipMemcpyDeviceToDevice, s));
    launch_prep_half_train((const double*)ctx->smp_x64.p, t.mu, ns, d, DP, ns, t.jx,
                           (unsigned short*)ctx->smp_img.p, (const float*)ctx->smp_xl2.p,
                           (unsigned long long*)ctx->smp_scr.p, ctx->xh_swz, s);
  }
  HIP_TRY(hipGetLastError());
  ctx->smp_kind = kmetric;
  ctx->smp_dp = DP;
  ctx->smp_swz = ctx->xh_swz;
  ctx->smp_n = ns;
  return KNN_OK;
}

static int check_train_args(int64_t n, int d, int class_cnt) {
  if (n <= 0) return knn_fail(KNN_ERR_ARG, "n_train must be > 0");
  if (n >= (int64_t)INT32_MAX - 4096)
    return knn_fail(KNN_ERR_ARG, "n_train per context must be < 2^31 (shard the train set)");
  if (d <= 0) return knn_fail(KNN_ERR_ARG, "dim must be > 0");
  if (class_cnt <= 0) return knn_fail(KNN_ERR_ARG, "class_cnt must be > 0");
  return KNN_OK;
}

extern "C" {

int knn_set_train(knn_ctx* ctx, const double* X, const int32_t* labels, int64_t n, int32_t d,
                  int32_t class_cnt) {
  int rc;
  if ((rc = device_guard(ctx))) return rc;
  if ((rc = check_train_args(n, d, class_cnt))) return rc;
  if (!X || !labels) return knn_fail(KNN_ERR_ARG, "null train pointer");
  // label range check (the reference indexes label_cnt[label] unchecked, cpp:330)
  for (int64_t i = 0; i < n; i++)
    if (labels[i] < 0 || labels[i] >= class_cnt)
      return knn_fail(KNN_ERR_ARG, "train label out of [0, class_cnt) at row " + std::to_string(i));
  if ((rc = ctx->X64_own.ensure((size_t)n * d * sizeof(double)))) return rc;
  if ((rc = ctx->lab_own.ensure((size_t)n * sizeof(int32_t)))) return rc;
  HIP_TRY(hipMemcpyAsync(ctx->X64_own.p, X, (size_t)n * d * sizeof(double),
                         hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipMemcpyAsync(ctx->lab_own.p, labels, (size_t)n * sizeof(int32_t),
                         hipMemcpyHostToDevice, ctx->stream));
  return build_train(ctx, (const double*)ctx->X64_own.p, (const int32_t*)ctx->lab_own.p, n, d,
                     class_cnt, 0);
}

int knn_set_train_device(knn_ctx* ctx, const double* dX, const int32_t* dlabels, int64_t n,
                         int32_t d, int32_t class_cnt, int64_t idx_offset) {
  int rc;
  if ((rc = device_guard(ctx))) return rc;
  if ((rc = check_train_args(n, d, class_cnt))) return rc;
  if (!dX || !dlabels) return knn_fail(KNN_ERR_ARG, "null train pointer");
  return build_train(ctx, dX, dlabels, n, d, class_cnt, idx_offset);
}

}  // extern "C"

// ---- timing ring (knn_set_timing): events of a call are read back lazily
// (mode 2: only ev[1] and ev[2], around the candidate kernel, are recorded)
static bool phase_timed(const TimedCall& tc, int p) { return tc.mode != 2 || p == 1; }
static void fold_timing(knn_ctx* ctx, TimedCall& tc) {
  if (!tc.pending) return;
  (void)hipEventSynchronize(tc.ev[tc.mode == 2 ? 2 : 4]);
  for (int p = 0; p < 4; p++) {
    float ms = 0.f;
    if (phase_timed(tc, p) && hipEventElapsedTime(&ms, tc.ev[p], tc.ev[p + 1]) == hipSuccess)
      ctx->tsum[p] += ms;
  }
  ctx->tcalls++;
  tc.pending = false;
}

static TimedCall* timing_slot(knn_ctx* ctx) {
  if (!ctx->timing) return nullptr;
  TimedCall& tc = ctx->ring[ctx->ring_next];
  fold_timing(ctx, tc);  // waits only when kTimingRing calls are still in flight
  ctx->ring_last = ctx->ring_next;
  ctx->ring_next = (ctx->ring_next + 1) % kTimingRing;
  tc.pending = true;
  tc.mode = ctx->timing;
  return &tc;
}
// the call's event e, if its timing mode records it
static hipEvent_t timing_ev(const TimedCall* tc, int e) {
  if (!tc || (tc->mode == 2 && e != 1 && e != 2)) return nullptr;
  return tc->ev[e];
}

// The deferred AUTO decision: once the last fp16 call has completed, its
// rescan count (written by the device into h_counts) decides whether the
// fp16 pass stays on for this train set.  Never waits.
static void auto_check(knn_ctx* ctx) {
  if (!ctx->auto_pending || hipEventQuery(ctx->done_ev) != hipSuccess) return;
  // AUTO retires the fp16 pass for this train set when a batch leaves more
  // than 1/16 of its queries to the rescan (data whose neighbour gaps are
  // too fine for fp16 operands): later batches take bf16x3
  if ((int64_t)ctx->h_counts[0] * 16 > ctx->auto_m) {
    if (ctx->auto_kind >= 5) ctx->i8_off = true;
    else ctx->fp16_off = true;
  }
  ctx->auto_pending = false;
}

// Core search: candidate pass + merge/re-rank/certify + the device-driven
// rescan.  Enqueue only: no host synchronisation on any path.
// Reference tie order (knn_select.hip, tie_order_kernel): which tied queries
// get the reference's own std::sort order.  Tuning key "ties": 0 none,
// 1 (default) those whose label the tie order could change (equal distances
// with different labels where two classes share the top count, or a tie
// across the k-th place within reach of the runner-up: finish_single),
// 2 every query with equal distances in its top k (neighbour indices in the
// reference's order too).
// (Partial lists stay ordered by (dist, global idx): the reference's order
// over the whole train set is restored after the merge, knn_tie_resolve_device.)
static int tie_mask_of(const knn_ctx* ctx, const Sink& sink) {
  if (sink.mode != MODE_SINGLE || sink.tie_defer) return 0;
  return ctx->tune.ties;
}

// Scratch of the reference-order passes: tie_scratch_bytes per concurrent
// workgroup, at most 32 workgroups and ~512 MB (at least one: n * 20 B); the
// passes loop over their queued queries, which are rare.
static int tie_workgroups(const knn_ctx* ctx, int64_t per) {
  return (int)std::max<int64_t>(
      1, std::min<int64_t>({(int64_t)32, (int64_t)ctx->cu_count, (512ll << 20) / per}));
}

// Queue and scratch of the reference-order pass for a sink with tie_mode set
// (every row's distance per workgroup; tied queries are rare, the pass loops
// over them).  zero_cnt: clear the queue's count here (knn_run_search clears
// it with the rescan counts instead).
struct TieScratch {
  int64_t per = 0;
  int nwg = 0;
};
static int tie_setup(knn_ctx* ctx, int64_t m, Sink& sink, TieScratch& ts, bool zero_cnt,
                     hipStream_t s) {
  if (!sink.tie_mode) return KNN_OK;
  int rc;
  ts.per = tie_scratch_bytes(ctx->train.n, ctx->class_cnt);
  ts.nwg = tie_workgroups(ctx, ts.per);
  if ((rc = ctx->tie_q.ensure((size_t)m * sizeof(int) + 16))) return rc;
  if ((rc = ctx->tie_ws.ensure((size_t)(ts.per * ts.nwg)))) return rc;
  if ((rc = ctx->rescan_cnt.ensure(4 * sizeof(int)))) return rc;
  sink.tie_q = (int*)ctx->tie_q.p;
  sink.tie_cnt = (int*)ctx->rescan_cnt.p + 2;
  if (zero_cnt) HIP_TRY(hipMemsetAsync(sink.tie_cnt, 0, sizeof(int), s));
  return KNN_OK;
}
// queries with exact distance ties: the reference's std::sort order
// excl (nullable): per-query excluded train rows (K sweep under exclusion)
static void tie_order(knn_ctx* ctx, const TieScratch& ts, int metric, const double* dQ,
                      const Sink& sink, hipStream_t s, const int64_t* excl = nullptr) {
  launch_tie_order(metric, ctx->train, dQ, sink.tie_q, sink.tie_cnt, ctx->class_cnt,
                   (unsigned char*)ctx->tie_ws.p, ts.per, ts.nwg, sink,
                   (unsigned long long*)ctx->totals.p + 2, s, excl);
}

static const KernelFacts kFacts = {cand_blocks_per_cu, s3q_blocks_per_cu, cand_queries_per_wave,
                                   cand_tile_rows, qres_supported};

// The train image the plan names, built on first use.
static int ensure_image(knn_ctx* ctx, const SearchPlan& p, hipStream_t s) {
  switch (p.image) {
    case IMG_I8: return ensure_i8(ctx, p.kmetric, s);
    case IMG_I8W: return ensure_i8_wide(ctx, s);
    case IMG_U16: return ensure_u16(ctx, s);
    case IMG_U16W: return ensure_u16_wide(ctx, s);
    case IMG_FP16: return ensure_fp16(ctx, s);
    case IMG_FP16_S3: return ensure_fp16_s3(ctx, s);
    case IMG_BF16X3: return ensure_bf16x3(ctx, s);
    default: return KNN_OK;
  }
}

int knn_run_search(knn_ctx* ctx, const double* dQ, int64_t m, int W, int metric,
                   const Sink& sink_in, hipStream_t s) {
  const TrainDev& t = ctx->train;
  int rc;
  auto_check(ctx);
  const PlanIn in{t.n, t.n_pad, t.d, t.DP, metric, m, W, ctx->precision, ctx->fp16_off,
                  ctx->i8_off, ctx->i8_ok, ctx->ord_P, ctx->ord_nb, ctx->cu_count,
                  ctx->timing != 0, ctx->tune, kFacts};
  const SearchPlan p = plan_search(in);
  if (!p.ok)
    return knn_fail(KNN_ERR_ARG, "no candidate kernel for this geometry (tuning overrides?)");
  if ((rc = ensure_image(ctx, p, s))) return rc;
  const int kmetric = p.kmetric, DP = p.DP, R = p.R, S = p.S, NL = p.NL, C = p.C, n_qt = p.n_qt;
  const int64_t m_pad = p.m_pad;
  const float* const images[] = {t.X32, (const float*)ctx->XB.p, (const float*)ctx->XH.p, nullptr,
                                 (const float*)ctx->XI.p, (const float*)ctx->XIW.p,
                                 (const float*)ctx->XU.p, (const float*)ctx->XUW.p};
  // the int8 passes (kernel metrics 5-7) share their query builder, centre
  // and scale; metric 8 takes the fp32 paths' query check and threshold fill
  const bool i8p = kmetric >= 5 && kmetric <= 7;
  // workspace, sized from the plan
  if ((rc = ctx->Q32.ensure((size_t)m_pad * DP * sizeof(float)))) return rc;
  if ((rc = ctx->qvalid.ensure((size_t)m_pad * sizeof(float)))) return rc;
  if ((rc = ctx->cand_v.ensure((size_t)m_pad * NL * R * sizeof(float)))) return rc;
  if ((rc = ctx->cand_i.ensure((size_t)m_pad * NL * R * sizeof(int)))) return rc;
  if (p.use_gthr && (rc = ctx->gthr.ensure((size_t)m_pad * kGthrSlots * sizeof(uint32_t))))
    return rc;
  if ((rc = ctx->rescan_q.ensure((size_t)m * sizeof(int) + 16))) return rc;
  if ((rc = ctx->rescan_tau.ensure((size_t)m * sizeof(double) + 16))) return rc;
  if ((rc = ctx->rescan_cnt.ensure(4 * sizeof(int)))) return rc;
  if ((rc = ctx->fr_cnt.ensure((size_t)p.cap * sizeof(int) + 16))) return rc;
  if ((rc = ctx->fr_buf.ensure((size_t)p.cap * kRescanCap * sizeof(int) + 16))) return rc;
  if ((rc = ctx->fr_q.ensure((size_t)p.cap * t.DP * sizeof(float) + 16))) return rc;
  if ((rc = ctx->fr_thr.ensure((size_t)p.cap * sizeof(float) + 16))) return rc;
  if ((rc = ctx->slow_q.ensure((size_t)m * sizeof(int) + 16))) return rc;
  if ((rc = ctx->rescan_mask.ensure((size_t)m * sizeof(unsigned long long) + 16))) return rc;
  if ((rc = ctx->rescan_nkeep.ensure((size_t)p.cap * sizeof(int) + 16))) return rc;
  Sink sink = sink_in;
  sink.tie_mode = tie_mask_of(ctx, sink_in);
  sink.tie_cnt = (int*)ctx->rescan_cnt.p + 2;  // zeroed with the rescan counts
  TieScratch ts;
  if ((rc = tie_setup(ctx, m, sink, ts, false, s))) return rc;

  ctx->last_kmetric = kmetric;
  ctx->geom[0] = (int64_t)(p.qres ? 2 * n_qt : n_qt) * S;  // (qres: workgroup tiles of 128 queries)
  ctx->geom[1] = S;
  ctx->geom[2] = R;
  ctx->last_nw = p.nw;
  ctx->geom[3] = C;
  memcpy(ctx->last_kernel, p.kernel, sizeof ctx->last_kernel);
  TimedCall* tc = timing_slot(ctx);
  if (hipEvent_t ev = timing_ev(tc, 0)) HIP_TRY(hipEventRecord(ev, s));
  // query operands: scale * 2^jx (q - mu), scale -2 for L2; a query whose
  // operands would leave the format's range (fp16: 65000, else 2^100) is
  // marked void and goes to the exact rescan
  const double qscale = metric == KNN_METRIC_L2 ? -2.0 : 1.0;
  float* qvalid = (float*)ctx->qvalid.p;
  // region order of the queries (resident kernels, metrics 4-6; knn_order.hip):
  // operand row p = query qperm[p], sorted by region; each query tile's
  // workgroups start their streams at the tile's region (qstart), and the
  // merge finds query q's lists at qpos[q]
  const int* qperm = nullptr;
  const int* qpos = nullptr;
  const int* qstart = nullptr;
  int64_t bcnt_clear = 0;  // block counts the int8 query builder clears after the sort
  if (p.query_order) {
    const int64_t nbc = region_sort_blocks(m) * kRegionMax;
    if ((rc = ctx->ord_qkey.ensure((size_t)m * sizeof(int)))) return rc;
    const size_t bcnt_cap = ctx->ord_bcnt.cap;
    if ((rc = ctx->ord_bcnt.ensure((size_t)nbc * sizeof(int)))) return rc;
    if (ctx->ord_bcnt.cap != bcnt_cap) ctx->ord_bcnt_zero = 0;  // (a new allocation)
    if ((rc = ctx->ord_qperm.ensure((size_t)m * sizeof(int)))) return rc;
    if ((rc = ctx->ord_qpos.ensure((size_t)m * sizeof(int)))) return rc;
    if ((rc = ctx->ord_qstart.ensure((size_t)m * sizeof(int)))) return rc;
    launch_region_sort_queries(dQ, t.mu, m, t.d, t.jx, (const unsigned short*)ctx->ord_img.p,
                               (const float*)ctx->ord_cnorm.p, ctx->ord_P,
                               (const int*)ctx->ord_rank.p, (const int*)ctx->ord_rstart.p,
                               p.ophase, (int*)ctx->ord_bcnt.p,
                               (int*)ctx->ord_tot.p, (int*)ctx->ord_qkey.p, (int*)ctx->ord_qperm.p,
                               (int*)ctx->ord_qpos.p, (int*)ctx->ord_qstart.p, s,
                               ctx->ord_bcnt_zero >= nbc);
    ctx->ord_bcnt_zero = 0;
    if (i8p) bcnt_clear = nbc;
    qperm = (const int*)ctx->ord_qperm.p;
    qpos = (const int*)ctx->ord_qpos.p;
    qstart = (const int*)ctx->ord_qstart.p;
  }
  if (!i8p)
    launch_query_check(dQ, t.mu, m, t.d, m_pad, qscale, t.jx,
                       kmetric == 4 ? 65000.0 : std::ldexp(1.0, 100), qvalid, s);
  if (p.image == IMG_U16W)
    launch_prep_u16_queries_wide(dQ, t.mu, m, t.d, DP, m_pad, ctx->u16_e,
                                 (unsigned short*)ctx->Q32.p, qvalid, s);
  else if (kmetric == 8)
    launch_prep_u16_queries(dQ, t.mu, m, t.d, DP, m_pad, ctx->u16_e, (unsigned short*)ctx->Q32.p,
                            qvalid, s);
  else if (i8p) {  // codes of the train set's grid; a query off it: valid 0 (rescan)
    launch_prep_i8_queries(dQ, t.mu, qscale, t.jx, DBL_MAX, (const double*)ctx->i8_cent.p, m, t.d,
                           DP, m_pad, ctx->i8_s, (signed char*)ctx->Q32.p, qvalid, s, qperm,
                           p.gthr_init ? (uint32_t*)ctx->gthr.p : nullptr, p.active,
                           (int*)ctx->ord_bcnt.p, bcnt_clear, (int*)ctx->rescan_cnt.p,
                           p.image == IMG_I8W);
    if (bcnt_clear) ctx->ord_bcnt_zero = bcnt_clear;
  } else if (p.s3h)
    launch_prep_half_tiled(dQ, t.mu, m, t.d, DP, m_pad, t.jx, -2.0, (unsigned short*)ctx->Q32.p,
                           nullptr, nullptr, qvalid, nullptr, s);
  else if (p.s3)
    launch_prep_split_tiled(dQ, t.mu, m, t.d, DP, m_pad, std::ldexp(qscale, t.jx),
                            (unsigned short*)ctx->Q32.p, nullptr, nullptr, s);
  else if (kmetric == 4)
    launch_prep_half_queries(dQ, t.mu, m, t.d, DP, m_pad, t.jx, (unsigned short*)ctx->Q32.p,
                             qvalid, s, qperm);
  else if (kmetric == 2 || kmetric == 3)
    launch_prep_split(dQ, t.mu, m, t.d, DP, m_pad, std::ldexp(qscale, t.jx),
                      (unsigned short*)ctx->Q32.p, 2 * DP, nullptr, nullptr, s);
  else
    launch_prep_queries(dQ, t.mu, m, t.d, DP, m_pad, qscale, t.jx, (float*)ctx->Q32.p, s);
  if (hipEvent_t ev = timing_ev(tc, 1); ev && !p.ev_ext) HIP_TRY(hipEventRecord(ev, s));
  CandLaunch cl{};
  if (p.ev_ext) {
    cl.ev_start = timing_ev(tc, 1);
    cl.ev_stop = timing_ev(tc, 2);
  }
  cl.metric = kmetric;
  cl.DP = DP;
  cl.R = R;
  cl.S = S;
  cl.n_qt = n_qt;
  cl.n_pad = t.n_pad;
  cl.X32 = images[p.image];
  cl.xinit = metric == 0 ? t.xinit_l2 : t.xinit_l1;
  cl.Q32 = (const float*)ctx->Q32.p;
  cl.out_v = (float*)ctx->cand_v.p;
  cl.out_i = (int*)ctx->cand_i.p;
  cl.ablate = p.ablate;
  cl.nw = p.nw;
  cl.qpb = p.qpb;
  cl.gthr = p.use_gthr ? (uint32_t*)ctx->gthr.p : nullptr;
  cl.gk = p.gk;
  cl.xsw = p.xsw;
  cl.qstart = qstart;
  cl.gmask = p.gmask;
  cl.qblk = p.qblk;
  if (p.gthr_init) {
    bool seeded = false;
    if (const int64_t ns = p.seed_rows) {
      // seeded thresholds (see seed_rows): the pre-pass over the sample
      if ((rc = ensure_sample(ctx, kmetric, DP, ns, s))) return rc;
      const int Ss = (int)std::max<int64_t>(1, std::min<int64_t>(16, ns / p.trows / 4));
      const int Us = 4 * Ss * R;  // quad lists: 4 per query per split
      if ((rc = ctx->smp_v.ensure((size_t)m_pad * Us * sizeof(float)))) return rc;
      if ((rc = ctx->smp_i.ensure((size_t)m_pad * Us * sizeof(int)))) return rc;
      CandLaunch cs = cl;
      cs.X32 = (const float*)ctx->smp_img.p;
      cs.n_pad = ns;
      cs.S = Ss;
      cs.out_v = (float*)ctx->smp_v.p;
      cs.out_i = (int*)ctx->smp_i.p;
      cs.gthr = nullptr;
      cs.ablate = 0;
      cs.ev_start = cs.ev_stop = nullptr;
      if (launch_cand(cs, s)) {
        launch_seed_gthr((const float*)ctx->smp_v.p, m_pad, Us, p.gk ? p.G * p.gk : 4 * R, p.active,
                         cl.gthr, s);
        seeded = true;
      }
    }
    if (!seeded && !i8p) launch_fill_gthr(cl.gthr, m_pad, p.active, s);
  }
  if (p.qres) {
    if (!launch_cand_qres((const unsigned short*)ctx->XT16.p, (const float*)ctx->XS16.p,
                          (const unsigned short*)ctx->Q32.p, DP, p.n_pad3, S, n_qt, cl.out_v, cl.out_i,
                          cl.gthr, p.gk, s, cl.ev_start, cl.ev_stop))
      return knn_fail(KNN_ERR_ARG, "no query-resident kernel for this dimension");
  } else if (p.s3h)
    launch_cand_s3h((const unsigned short*)ctx->XT16.p, (const float*)ctx->XS16.p,
                    (const unsigned short*)ctx->Q32.p, DP, p.n_pad3, R, S, n_qt, cl.out_v, cl.out_i,
                    cl.ablate, p.s3q, cl.gthr, p.gk, s, p.s3gq);
  else if (p.s3)
    launch_cand_s3((const unsigned short*)ctx->XB.p, (const float*)ctx->XS.p,
                   (const unsigned short*)ctx->Q32.p, DP, p.n_pad3, R, S, n_qt, cl.out_v, cl.out_i,
                   cl.ablate, s, p.s3gq);
  else if (!launch_cand(cl, s))
    return knn_fail(KNN_ERR_ARG, "no candidate kernel for this geometry (tuning overrides?)");
  HIP_TRY(hipGetLastError());
  if (hipEvent_t ev = timing_ev(tc, 2); ev && !p.ev_ext) HIP_TRY(hipEventRecord(ev, s));
  // the rescan / tie counters (the int8 query builder cleared them already)
  if (!i8p) HIP_TRY(hipMemsetAsync(ctx->rescan_cnt.p, 0, 4 * sizeof(int), s));
  // per-split certification: a query failing only through some splits'
  // lists rescans just those splits' rows (knn_select.hip)
  SplitMap sm;
  sm.S = S <= 64 ? S : 0;
  sm.lps = p.lps;
  sm.trows = p.trows;
  sm.cap = p.cap;
  sm.mask = (unsigned long long*)ctx->rescan_mask.p;
  sm.nkeep = (int*)ctx->rescan_nkeep.p;
  sm.keep = (int*)ctx->fr_buf.p;
  RescanPrep rp;
  rp.mu = t.mu;
  rp.x2max = t.x2max;
  rp.x1max = t.x1max;
  rp.jx = t.jx;
  rp.DP = t.DP;
  rp.f_err = err_factor(metric, t.DP);
  rp.qf = (float*)ctx->fr_q.p;
  rp.thr = (float*)ctx->fr_thr.p;
  rp.fcnt = (int*)ctx->fr_cnt.p;
  rp.cap = p.abl ? 0 : p.cap;
  if (p.i8resc) {
    if ((rc = ctx->rescan_qc8.ensure((size_t)p.cap * 256 + 16))) return rc;
    if ((rc = ctx->rescan_t8.ensure((size_t)p.cap * sizeof(long long) + 16))) return rc;
    rp.qc8 = (signed char*)ctx->rescan_qc8.p;
    rp.t8 = (long long*)ctx->rescan_t8.p;
  }
  if (kmetric == 8) {
    // 16-bit fixed-point L1 proxies are in units of 2^-e; their error is the
    // two vectors' measured coding errors (the merge rebuilds the query's
    // codes) plus err_factor(8)'s fp64 rounding terms; above 256 dims the
    // sums' conversion to float adds fix16_wide_round code units (0 below)
    TrainDev tu = t;
    tu.jx = ctx->u16_e;
    ProxyScale ps{qvalid, 0.0, 0.0, false, nullptr, qpos};
    ps.u16dx = ctx->u16_dx + fix16_wide_round(DP);
    launch_merge_rerank(metric, (const float*)ctx->cand_v.p, (const int*)ctx->cand_i.p, NL, R, tu,
                        dQ, m, W, C, err_factor(8, DP), ps, cl.gthr, sink, (int*)ctx->rescan_q.p,
                        (double*)ctx->rescan_tau.p, (int*)ctx->rescan_cnt.p, sm, rp, s);
  } else if (i8p) {
    // int8 proxies are exact up to +1 (the odd-norm half of the seed): the
    // merge sees the pass's own centre and scale (codes (x - cent/2^s) 2^s),
    // an absolute error of one code unit (DP x up / DP) and each query's
    // own coding error (off the grid / beyond the code range), measured
    TrainDev t8 = t;
    t8.mu = (const double*)ctx->i8_cent.p + t.d;
    t8.jx = ctx->i8_s;
    t8.x2max = ctx->i8_x2max;
    t8.DP = DP;
    launch_merge_rerank(metric, (const float*)ctx->cand_v.p, (const int*)ctx->cand_i.p, NL, R, t8,
                        dQ, m, W, C, 0.0,
                        // (metric 7: L1 proxies are exact on the grid and void off it;
                        // the re-rank reads the fp64 rows)
                        kmetric == 7
                            ? ProxyScale{qvalid, 0.0, 0.0, false, (const double*)ctx->i8_cent.p, qpos}
                            : ProxyScale{qvalid, 0.0, 1.0 / DP, false, (const double*)ctx->i8_cent.p, qpos,
                                         (const signed char*)ctx->XI.p, DP + 16, DP, p.i8_swz},
                        cl.gthr, sink,
                        (int*)ctx->rescan_q.p, (double*)ctx->rescan_tau.p, (int*)ctx->rescan_cnt.p,
                        sm, rp, s);
  } else {
    launch_merge_rerank(metric, (const float*)ctx->cand_v.p, (const int*)ctx->cand_i.p, NL, R, t,
                        dQ, m, W, C, err_factor(kmetric, DP),
                        kmetric == 4 ? ProxyScale{qvalid, 0x1p-14, 0x1p-28, true, nullptr, qpos}
                                     : ProxyScale{qvalid, 0x1p-125, 0x1p-124, false, nullptr, qpos},
                        cl.gthr, sink, (int*)ctx->rescan_q.p, (double*)ctx->rescan_tau.p,
                        (int*)ctx->rescan_cnt.p, sm, rp, s);
  }
  HIP_TRY(hipGetLastError());
  if (hipEvent_t ev = timing_ev(tc, 3)) HIP_TRY(hipEventRecord(ev, s));
  // rescan of uncertified queries, sized on the device (knn_select.hip)
  RescanBufs rb{};
  rb.q = (int*)ctx->rescan_q.p;
  rb.tau = (double*)ctx->rescan_tau.p;
  rb.cnt = (int*)ctx->rescan_cnt.p;
  rb.qf = (float*)ctx->fr_q.p;
  rb.thr = (float*)ctx->fr_thr.p;
  rb.fcnt = (int*)ctx->fr_cnt.p;
  rb.buf = (int*)ctx->fr_buf.p;
  rb.slow_q = (int*)ctx->slow_q.p;
  rb.counts = ctx->d_counts;
  rb.totals = (unsigned long long*)ctx->totals.p;
  rb.mask = sm.mask;
  rb.nkeep = sm.nkeep;
  rb.S = sm.S;
  rb.trows = sm.trows;
  rb.cus = ctx->cu_count;
  if (p.i8resc) {
    rb.qc8 = rp.qc8;
    rb.t8 = rp.t8;
    rb.i8img = (const signed char*)ctx->XI.p;
    rb.i8rb = DP + 16;
    rb.i8dp = DP;
  }
  launch_rescan(metric, t, dQ, rb, rp.cap, W, err_factor(metric, t.DP), sink,
                p.abl ? 0 : (int)std::min<int64_t>(m, ctx->cu_count), s);
  // (without the full-scan launch nothing writes this call's counts)
  if (p.abl) launch_fill_i32(ctx->d_counts, 2, 0, s);
  if (sink.tie_mode && !p.abl) tie_order(ctx, ts, metric, dQ, sink, s);
  HIP_TRY(hipGetLastError());
  if (hipEvent_t ev = timing_ev(tc, 4)) HIP_TRY(hipEventRecord(ev, s));
  HIP_TRY(hipEventRecord(ctx->done_ev, s));
  ctx->auto_pending = p.auto_arm;
  ctx->auto_kind = kmetric;
  ctx->auto_m = m;
  return KNN_OK;
}

// k > kMaxK: the exact large-k path (knn_select.hip, large_k_kernel); the
// scratch (every row's distance per workgroup) is capped at ~8 GB.
static int run_large_k(knn_ctx* ctx, const double* dQ, int64_t m, int W, int metric,
                       const Sink& sink_in, hipStream_t s) {
  const TrainDev& t = ctx->train;
  Sink sink = sink_in;
  sink.tie_mode = tie_mask_of(ctx, sink_in);
  int rc;
  TieScratch ts;  // tied queries: queued by large_k_kernel for the reference-order pass
  if ((rc = tie_setup(ctx, m, sink, ts, true, s))) return rc;
  const int64_t per = large_k_scratch_bytes(t.n, W, ctx->class_cnt);
  const int64_t nwg = std::max<int64_t>(
      1, std::min<int64_t>({m, 2 * (int64_t)ctx->cu_count, (8ll << 30) / per}));
  if ((rc = ctx->lk.ensure((size_t)(per * nwg)))) return rc;
  snprintf(ctx->last_kernel, sizeof ctx->last_kernel, "large_k_kernel<%d>", metric);
  ctx->last_kmetric = -1;
  launch_large_k(metric, t, dQ, m, W, ctx->class_cnt, (unsigned char*)ctx->lk.p, per, (int)nwg,
                 sink, s);
  if (sink.tie_mode) tie_order(ctx, ts, metric, dQ, sink, s);
  launch_fill_i32(ctx->d_counts, 2, 0, s);  // exact path: no query fails certification
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(ctx->done_ev, s));
  ctx->auto_pending = false;  // done_ev / h_counts now belong to this call
  return KNN_OK;
}

// K sweep (knn_sweep.hip): ks is a host array in any order, duplicates allowed.
int knn_sweep_check_ks(const int32_t* ks, int32_t nk, int64_t n, int32_t* kmax) {
  if (nk < 1 || nk > 4096)
    return knn_fail(KNN_ERR_ARG, "nk = " + std::to_string(nk) + " must be in [1, 4096]");
  if (!ks) return knn_fail(KNN_ERR_ARG, "null ks");
  int32_t mx = 0;
  for (int32_t i = 0; i < nk; i++) {
    if (ks[i] < 0)
      return knn_fail(KNN_ERR_ARG, "ks[" + std::to_string(i) + "] = " + std::to_string(ks[i]) +
                                       " must be >= 0");
    if (ks[i] > n)
      return knn_fail(KNN_ERR_ARG, "ks[" + std::to_string(i) + "] = " + std::to_string(ks[i]) +
                                       " exceeds " + std::to_string(n) +
                                       " (the rows available to vote over)");
    mx = std::max(mx, ks[i]);
  }
  *kmax = mx;
  return KNN_OK;
}

// the list of K on the device (a copy from pageable host memory: staged by
// the runtime before the call returns) and the zeroed correct counts
static int sweep_upload(knn_ctx* ctx, const int32_t* ks, int32_t nk, int64_t* d_correct,
                        hipStream_t s) {
  int rc;
  if ((rc = ctx->sw_ks.ensure((size_t)nk * sizeof(int32_t)))) return rc;
  HIP_TRY(hipMemcpyAsync(ctx->sw_ks.p, ks, (size_t)nk * sizeof(int32_t), hipMemcpyHostToDevice, s));
  if (d_correct) HIP_TRY(hipMemsetAsync(d_correct, 0, (size_t)nk * sizeof(int64_t), s));
  return KNN_OK;
}

// the prefix votes over a call's finished rows in the context's vote mode
// (knn_sweep.hip / knn_wvote.hip)
static void sweep_votes(knn_ctx* ctx, const int64_t* idx, const double* dist, int64_t m, int kmax,
                        const int* dks, int nk, int32_t* d_labels, const int32_t* d_truth,
                        int64_t* d_correct, hipStream_t s) {
  if (ctx->vote == KNN_VOTE_DISTANCE)
    launch_wvote_sweep(idx, dist, m, kmax, ctx->train.lab, ctx->idx_off, dks, nk, d_labels,
                       d_truth, (unsigned long long*)d_correct, ctx->cu_count, s);
  else
    launch_sweep_vote(idx, m, kmax, ctx->train.lab, ctx->idx_off, dks, nk, d_labels, d_truth,
                      (unsigned long long*)d_correct, ctx->cu_count, s);
}

static int check_query_args(knn_ctx* ctx, int64_t m, int32_t k, int32_t metric) {
  if (!ctx->trained) return knn_fail(KNN_ERR_STATE, "classify before set_train");
  if (m < 0) return knn_fail(KNN_ERR_ARG, "m must be >= 0");
  if (m >= (int64_t)INT32_MAX) return knn_fail(KNN_ERR_ARG, "m must be < 2^31 per call");
  if (k < 0) return knn_fail(KNN_ERR_ARG, "k must be >= 0");
  if (k > ctx->train.n)
    return knn_fail(KNN_ERR_ARG, "k exceeds n_train (the reference reads past its array, cpp:328)");
  if (metric != KNN_METRIC_L2 && metric != KNN_METRIC_L1)
    return knn_fail(KNN_ERR_ARG, "metric must be 0 (L2) or 1 (L1)");
  return KNN_OK;
}

// ---- the K sweep's one body: plain, under row exclusion (knn_loo.hip) and
// under group exclusion (knn_lgo.hip)

// what a sweep's queries leave out of the train set
struct Excl {
  enum Kind { NONE, ROW, GROUP } kind = NONE;
  const int64_t* row = nullptr;     // ROW: one global train index per query (-1 = none)
  const int32_t* qgroup = nullptr;  // GROUP: one id of ctx->groups per query (-1 = none)
  static Excl of_row(const int64_t* d_excl) {  // (a null array excludes nothing)
    return d_excl ? Excl{ROW, d_excl, nullptr} : Excl{};
  }
  static Excl of_group(const int32_t* d_qgroup) {
    return d_qgroup ? Excl{GROUP, nullptr, d_qgroup} : Excl{};
  }
};

// knn_classify_sweep_device / _excl_device / _gexcl_device on stream s.  Under
// exclusion a query may lose `drop` rows (1, or the largest group), so one
// search at kmax + drop goes into internal rows and is compacted into the
// kmax-entry rows of the reduced sets; the plain sweep searches at kmax
// straight into those rows.
static int sweep_run(knn_ctx* ctx, const double* dQ, int64_t m, const Excl& ex, const int32_t* ks,
                     int32_t nk, int32_t metric, int32_t* d_labels, const int32_t* d_truth,
                     int64_t* d_correct, int64_t* d_idx, double* d_dist, int32_t* d_flags,
                     hipStream_t s) {
  int rc;
  if ((rc = check_query_args(ctx, m, 0, metric))) return rc;
  if (ex.kind == Excl::GROUP && !ctx->groups)
    return knn_fail(KNN_ERR_STATE, "sweep under group exclusion before knn_set_groups");
  const TrainDev& t = ctx->train;
  const int drop = ex.kind == Excl::GROUP ? ctx->gmax : ex.kind == Excl::ROW ? 1 : 0;
  int32_t kmax = 0;
  if ((rc = knn_sweep_check_ks(ks, nk, t.n - drop, &kmax))) return rc;
  if ((d_truth != nullptr) != (d_correct != nullptr))
    return knn_fail(KNN_ERR_ARG, "d_truth and d_correct go together (both or neither)");
  if (!d_labels) return knn_fail(KNN_ERR_ARG, "null labels output");
  if ((rc = sweep_upload(ctx, ks, nk, d_correct, s))) return rc;
  if (m == 0) return KNN_OK;
  if (!dQ) return knn_fail(KNN_ERR_ARG, "null query pointer");
  const int* dks = (const int*)ctx->sw_ks.p;
  if (kmax == 0) {  // every K is 0: no neighbour is read, max_label stays -1 (cpp:324)
    launch_sweep_vote(nullptr, m, 0, t.lab, ctx->idx_off, dks, nk, d_labels, d_truth,
                      (unsigned long long*)d_correct, ctx->cu_count, s);
    if (d_flags) launch_fill_i32(d_flags, m, 0, s);
    HIP_TRY(hipGetLastError());
    return KNN_OK;
  }
  const bool excl = ex.kind != Excl::NONE;
  const int k1 = kmax + drop;  // <= n
  if ((rc = ctx->sw_lab.ensure((size_t)m * sizeof(int32_t)))) return rc;
  if (excl && (rc = ctx->loo_idx.ensure((size_t)m * k1 * sizeof(int64_t)))) return rc;
  if (excl && (rc = ctx->loo_dist.ensure((size_t)m * k1 * sizeof(double)))) return rc;
  if (excl && (rc = ctx->loo_flags.ensure((size_t)m * sizeof(int32_t)))) return rc;
  if (!d_idx && (rc = ctx->sw_idx.ensure((size_t)m * kmax * sizeof(int64_t)))) return rc;
  if (!d_dist && (rc = ctx->sw_dist.ensure((size_t)m * kmax * sizeof(double)))) return rc;
  if (!d_flags && (rc = ctx->sw_flags.ensure((size_t)m * sizeof(int32_t)))) return rc;
  // the rows the sweep always keeps (idx, dist, flags), at kmax
  Sink out{};
  out.mode = MODE_SINGLE;
  out.k = kmax;
  out.idx_off = ctx->idx_off;
  out.labels = (int32_t*)ctx->sw_lab.p;
  out.idx = d_idx ? d_idx : (int64_t*)ctx->sw_idx.p;
  out.dist = d_dist ? d_dist : (double*)ctx->sw_dist.p;
  out.flags = d_flags ? d_flags : (int32_t*)ctx->sw_flags.p;
  out.tie_defer = 1;  // the search neither queues ties nor runs the reference-order pass
  Sink sink = out;    // the rows the search writes
  if (excl) {
    sink.k = k1;
    sink.idx = (int64_t*)ctx->loo_idx.p;
    sink.dist = (double*)ctx->loo_dist.p;
    sink.flags = (int32_t*)ctx->loo_flags.p;
  }
  const int W = (int)std::min<int64_t>((int64_t)k1 + 1, t.n);
  rc = k1 > kMaxK ? run_large_k(ctx, dQ, m, W, metric, sink, s)
                  : knn_run_search(ctx, dQ, m, W, metric, sink, s);
  if (rc) return rc;
  if (ex.kind == Excl::ROW)
    launch_loo_drop(sink.dist, sink.idx, sink.flags, ex.row, m, kmax, t.lab, ctx->idx_off, t.n,
                    out.dist, out.idx, out.flags, ctx->cu_count, s);
  else if (ex.kind == Excl::GROUP)
    launch_lgo_drop(sink.dist, sink.idx, sink.flags, ex.qgroup, ctx->groups, m, kmax, k1, t.lab,
                    ctx->idx_off, t.n, out.dist, out.idx, out.flags, ctx->cu_count, s);
  // queries whose label at some K of the list the reference's tie order could
  // change -> the tie queue -> the reference-order pass over the whole top
  // kmax (std::sort over each query's remaining records)
  if (ctx->tune.ties) {
    out.tie_mode = ctx->tune.ties;
    TieScratch ts;
    if ((rc = tie_setup(ctx, m, out, ts, true, s))) return rc;
    launch_sweep_tie_scan(out.dist, out.idx, out.flags, m, kmax, t.lab, ctx->idx_off, dks, nk,
                          out.tie_mode, out.tie_q, out.tie_cnt, ctx->cu_count, s);
    if (ex.kind == Excl::GROUP)
      launch_tie_order_group(metric, t, dQ, out.tie_q, out.tie_cnt, ctx->class_cnt,
                             (unsigned char*)ctx->tie_ws.p, ts.per, ts.nwg, out,
                             (unsigned long long*)ctx->totals.p + 2, s, ex.qgroup, ctx->groups);
    else
      tie_order(ctx, ts, metric, dQ, out, s, ex.row);
  }
  sweep_votes(ctx, out.idx, out.dist, m, kmax, dks, nk, d_labels, d_truth, d_correct, s);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(ctx->done_ev, s));  // the call ends after the vote
  return KNN_OK;
}

// ---- per-class evaluation (knn_eval.hip)
// The sweep into d_labels or, without them, the context's workspace, then the
// confusion pass over those labels against d_truth (d_conf / d_unl nullable:
// none asked for, no pass).  zero: the call clears d_conf / d_unl first, as
// the sweep clears d_correct; the callers that walk the train set in batches
// sum them on the device without it.
static int sweep_eval_run(knn_ctx* ctx, const double* dQ, int64_t m, const Excl& ex,
                          const int32_t* ks, int32_t nk, int32_t metric, int32_t* d_labels,
                          const int32_t* d_truth, int64_t* d_correct, int64_t* d_idx,
                          double* d_dist, int32_t* d_flags, int64_t* d_conf, int64_t* d_unl,
                          bool zero, hipStream_t s) {
  int rc;
  const size_t cc = (size_t)ctx->class_cnt * ctx->class_cnt;
  if (nk >= 1 && nk <= 4096) {  // (a bad nk is reported by the sweep's own check)
    if (zero && d_conf) HIP_TRY(hipMemsetAsync(d_conf, 0, (size_t)nk * cc * sizeof(int64_t), s));
    if (zero && d_unl) HIP_TRY(hipMemsetAsync(d_unl, 0, (size_t)nk * sizeof(int64_t), s));
  }
  int32_t* L = d_labels;
  if (!L) {
    const size_t cells = (size_t)std::max<int64_t>(m, 1) * (size_t)std::max(nk, 1);
    if ((rc = ctx->ev_lab.ensure(cells * sizeof(int32_t)))) return rc;
    L = (int32_t*)ctx->ev_lab.p;
  }
  rc = sweep_run(ctx, dQ, m, ex, ks, nk, metric, L, d_correct ? d_truth : nullptr, d_correct,
                 d_idx, d_dist, d_flags, s);
  if (rc || m == 0 || (!d_conf && !d_unl)) return rc;
  launch_eval_confusion(L, nk, m, d_truth, ctx->class_cnt, (unsigned long long*)d_conf,
                        (unsigned long long*)d_unl, s);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(ctx->done_ev, s));  // the call ends after the confusion pass
  return KNN_OK;
}

// the query form (knn_classify_sweep_eval_device's body): d_truth required
static int sweep_eval(knn_ctx* ctx, const double* dQ, int64_t m, const int64_t* d_excl,
                      const int32_t* ks, int32_t nk, int32_t metric, int32_t* d_labels,
                      const int32_t* d_truth, int64_t* d_correct, int64_t* d_conf, int64_t* d_unl,
                      hipStream_t s) {
  int rc;
  if ((rc = check_query_args(ctx, m, 0, metric))) return rc;
  int32_t kmax = 0;
  if ((rc = knn_sweep_check_ks(ks, nk, ctx->train.n, &kmax))) return rc;
  if (!d_truth)
    return knn_fail(KNN_ERR_ARG, "null d_truth (the evaluation needs the queries' true labels)");
  return sweep_eval_run(ctx, dQ, m, Excl::of_row(d_excl), ks, nk, metric, d_labels, d_truth,
                        d_correct, nullptr, nullptr, nullptr, d_conf, d_unl, true, s);
}

// leave-one-out (own_group false) / leave-group-out over train rows [row0,
// row0 + rows): the rows are the queries, each excludes itself / its own
// group and its own label is its truth
int knn_sweep_rows(knn_ctx* ctx, int64_t row0, int64_t rows, bool own_group, const int32_t* ks,
                   int32_t nk, int32_t metric, int32_t* d_labels, int64_t* d_correct,
                   int64_t* d_idx, double* d_dist, int32_t* d_flags, int64_t* d_conf,
                   int64_t* d_unl, bool zero, hipStream_t s) {
  int rc;
  if (!ctx->trained)
    return knn_fail(KNN_ERR_STATE, own_group ? "leave-group-out sweep before set_train"
                                             : "leave-one-out sweep before set_train");
  if (own_group && !ctx->groups)
    return knn_fail(KNN_ERR_STATE, "leave-group-out sweep before knn_set_groups");
  const TrainDev& t = ctx->train;
  if (row0 < 0 || rows < 0 || row0 > t.n || rows > t.n - row0)
    return knn_fail(KNN_ERR_ARG, "rows [" + std::to_string(row0) + ", " +
                                     std::to_string(row0) + " + " + std::to_string(rows) +
                                     ") outside the train set [0, " + std::to_string(t.n) + ")");
  // query i is train row row0 + i
  const size_t r1 = (size_t)std::max<int64_t>(rows, 1);
  Excl ex;
  if (own_group) {
    if ((rc = ctx->lgo_qg.ensure(r1 * sizeof(int32_t)))) return rc;
    launch_lgo_self((int32_t*)ctx->lgo_qg.p, ctx->groups, rows, row0, s);
    ex = Excl::of_group((const int32_t*)ctx->lgo_qg.p);
  } else {
    if ((rc = ctx->loo_excl.ensure(r1 * sizeof(int64_t)))) return rc;
    launch_loo_self((int64_t*)ctx->loo_excl.p, rows, ctx->idx_off + row0, s);
    ex = Excl::of_row((const int64_t*)ctx->loo_excl.p);
  }
  HIP_TRY(hipGetLastError());
  return sweep_eval_run(ctx, t.X64 + row0 * t.d, rows, ex, ks, nk, metric, d_labels,
                        t.lab + row0, d_correct, d_idx, d_dist, d_flags, d_conf, d_unl, zero, s);
}

// ---- the host twins: staging in the context's buffers on its own stream

// knn_classify_sweep / knn_classify_sweep_eval after their argument checks:
// queries and truth up, the sweep (eval: through sweep_eval), the outputs the
// caller asked for down, one wait
static int host_sweep(knn_ctx* ctx, const double* Q, int64_t m, const int32_t* ks, int32_t nk,
                      int32_t kmax, int32_t metric, bool eval, int32_t* out_labels,
                      const int32_t* truth, int64_t* out_correct, int64_t* out_conf,
                      int64_t* out_unl, int64_t* out_idx, double* out_dist, int32_t* out_flags) {
  int rc;
  const int d = ctx->train.d;
  const size_t cc = (size_t)ctx->class_cnt * ctx->class_cnt;
  const size_t m1 = (size_t)std::max<int64_t>(m, 1), mk = (size_t)m * kmax;
  if ((rc = ctx->Q64.ensure(m1 * d * sizeof(double)))) return rc;
  if (out_labels && (rc = ctx->sw_out.ensure(m1 * nk * sizeof(int32_t)))) return rc;
  if (truth && (rc = ctx->sw_truth.ensure(m1 * sizeof(int32_t)))) return rc;
  if (out_correct && (rc = ctx->sw_corr.ensure((size_t)nk * sizeof(int64_t)))) return rc;
  if (out_conf && (rc = ctx->ev_conf.ensure((size_t)nk * cc * sizeof(int64_t)))) return rc;
  if (out_unl && (rc = ctx->ev_unl.ensure((size_t)nk * sizeof(int64_t)))) return rc;
  if (out_idx && (rc = ctx->o_idx.ensure(mk * sizeof(int64_t)))) return rc;
  if (out_dist && (rc = ctx->o_dist.ensure(mk * sizeof(double)))) return rc;
  if (out_flags && (rc = ctx->o_flags.ensure(m1 * sizeof(int32_t)))) return rc;
  hipStream_t s = ctx->stream;
  if (m > 0) {
    HIP_TRY(hipMemcpyAsync(ctx->Q64.p, Q, (size_t)m * d * sizeof(double), hipMemcpyHostToDevice, s));
    if (truth)
      HIP_TRY(hipMemcpyAsync(ctx->sw_truth.p, truth, (size_t)m * sizeof(int32_t),
                             hipMemcpyHostToDevice, s));
  }
  const double* dQ = (const double*)ctx->Q64.p;
  int32_t* d_labels = out_labels ? (int32_t*)ctx->sw_out.p : nullptr;
  const int32_t* d_truth = truth ? (const int32_t*)ctx->sw_truth.p : nullptr;
  int64_t* d_correct = out_correct ? (int64_t*)ctx->sw_corr.p : nullptr;
  if (eval)
    rc = sweep_eval(ctx, dQ, m, nullptr, ks, nk, metric, d_labels, d_truth, d_correct,
                    out_conf ? (int64_t*)ctx->ev_conf.p : nullptr,
                    out_unl ? (int64_t*)ctx->ev_unl.p : nullptr, s);
  else
    rc = sweep_run(ctx, dQ, m, Excl{}, ks, nk, metric, d_labels, d_truth, d_correct,
                   out_idx ? (int64_t*)ctx->o_idx.p : nullptr,
                   out_dist ? (double*)ctx->o_dist.p : nullptr,
                   out_flags ? (int32_t*)ctx->o_flags.p : nullptr, s);
  if (rc) return rc;
  if ((rc = copy_back(out_labels, ctx->sw_out.p, (size_t)m * nk * sizeof(int32_t), s))) return rc;
  if ((rc = copy_back(out_correct, ctx->sw_corr.p, (size_t)nk * sizeof(int64_t), s))) return rc;
  if ((rc = copy_back(out_conf, ctx->ev_conf.p, (size_t)nk * cc * sizeof(int64_t), s))) return rc;
  if ((rc = copy_back(out_unl, ctx->ev_unl.p, (size_t)nk * sizeof(int64_t), s))) return rc;
  if ((rc = copy_back(out_flags, ctx->o_flags.p, (size_t)m * sizeof(int32_t), s))) return rc;
  if ((rc = copy_back(out_idx, ctx->o_idx.p, mk * sizeof(int64_t), s))) return rc;
  if ((rc = copy_back(out_dist, ctx->o_dist.p, mk * sizeof(double), s))) return rc;
  HIP_TRY(hipStreamSynchronize(s));
  return KNN_OK;
}

// knn_loo_sweep / knn_loo_sweep_eval / knn_lgo_sweep after their argument
// checks: knn_sweep_rows over the whole train set in fixed batches (the
// workspace does not grow with n; without out_labels no [nk][n] array exists
// anywhere).  conf / unl are summed over the batches on the device, correct
// on the host.
static int host_rows_walk(knn_ctx* ctx, bool own_group, const int32_t* ks, int32_t nk,
                          int32_t kmax, int32_t metric, int32_t* out_labels,
                          int64_t* out_correct, int64_t* out_conf, int64_t* out_unl,
                          int64_t* out_idx, double* out_dist, int32_t* out_flags) {
  int rc;
  const int64_t n = ctx->train.n;
  const int64_t B = std::min<int64_t>(n, 16384);
  const int64_t nb = (n + B - 1) / B;
  const size_t bk = (size_t)B * kmax;
  const size_t cc = (size_t)ctx->class_cnt * ctx->class_cnt;
  if ((rc = ctx->sw_out.ensure((size_t)B * nk * sizeof(int32_t)))) return rc;
  if (out_correct && (rc = ctx->sw_corr.ensure((size_t)nk * sizeof(int64_t)))) return rc;
  if (out_conf && (rc = ctx->ev_conf.ensure((size_t)nk * cc * sizeof(int64_t)))) return rc;
  if (out_unl && (rc = ctx->ev_unl.ensure((size_t)nk * sizeof(int64_t)))) return rc;
  if (out_idx && (rc = ctx->o_idx.ensure(bk * sizeof(int64_t)))) return rc;
  if (out_dist && (rc = ctx->o_dist.ensure(bk * sizeof(double)))) return rc;
  if (out_flags && (rc = ctx->o_flags.ensure((size_t)B * sizeof(int32_t)))) return rc;
  hipStream_t s = ctx->stream;
  if (out_conf) HIP_TRY(hipMemsetAsync(ctx->ev_conf.p, 0, (size_t)nk * cc * sizeof(int64_t), s));
  if (out_unl) HIP_TRY(hipMemsetAsync(ctx->ev_unl.p, 0, (size_t)nk * sizeof(int64_t), s));
  std::vector<int64_t> hc(out_correct ? (size_t)nb * nk : 0, 0);  // per batch, summed at the end
  for (int64_t b = 0; b < nb; b++) {
    const int64_t r0 = b * B, rows = std::min(B, n - r0);
    rc = knn_sweep_rows(ctx, r0, rows, own_group, ks, nk, metric, (int32_t*)ctx->sw_out.p,
                        out_correct ? (int64_t*)ctx->sw_corr.p : nullptr,
                        out_idx ? (int64_t*)ctx->o_idx.p : nullptr,
                        out_dist ? (double*)ctx->o_dist.p : nullptr,
                        out_flags ? (int32_t*)ctx->o_flags.p : nullptr,
                        out_conf ? (int64_t*)ctx->ev_conf.p : nullptr,
                        out_unl ? (int64_t*)ctx->ev_unl.p : nullptr, false, s);
    if (rc) return rc;
    // the batch's labels [nk][rows] -> columns [r0, r0 + rows) of [nk][n]
    if (out_labels)
      HIP_TRY(hipMemcpy2DAsync(out_labels + r0, (size_t)n * sizeof(int32_t), ctx->sw_out.p,
                               (size_t)rows * sizeof(int32_t), (size_t)rows * sizeof(int32_t),
                               (size_t)nk, hipMemcpyDeviceToHost, s));
    if ((rc = copy_back(out_correct ? hc.data() + b * nk : nullptr, ctx->sw_corr.p,
                        (size_t)nk * sizeof(int64_t), s)))
      return rc;
    if ((rc = copy_back(out_flags ? out_flags + r0 : nullptr, ctx->o_flags.p,
                        (size_t)rows * sizeof(int32_t), s)))
      return rc;
    if ((rc = copy_back(out_idx ? out_idx + r0 * kmax : nullptr, ctx->o_idx.p,
                        (size_t)rows * kmax * sizeof(int64_t), s)))
      return rc;
    if ((rc = copy_back(out_dist ? out_dist + r0 * kmax : nullptr, ctx->o_dist.p,
                        (size_t)rows * kmax * sizeof(double), s)))
      return rc;
  }
  if ((rc = copy_back(out_conf, ctx->ev_conf.p, (size_t)nk * cc * sizeof(int64_t), s))) return rc;
  if ((rc = copy_back(out_unl, ctx->ev_unl.p, (size_t)nk * sizeof(int64_t), s))) return rc;
  HIP_TRY(hipStreamSynchronize(s));
  if (out_correct)
    for (int32_t j = 0; j < nk; j++) {
      out_correct[j] = 0;
      for (int64_t b = 0; b < nb; b++) out_correct[j] += hc[(size_t)b * nk + j];
    }
  return KNN_OK;
}

// ---- F-fold cross-validated K sweep on fold shards (knn_fold.hip)

constexpr int64_t kFoldBatch = 16384;  // queries per batch, as the leave-one-out walk

// knn_kfold_sweep* up to the first launch: the state, the list of K against
// the rows the smallest remaining set holds, the metric
static int fold_check(knn_ctx* ctx, const int32_t* ks, int32_t nk, int32_t metric, int32_t* kmax) {
  int rc;
  if (!ctx->trained) return knn_fail(KNN_ERR_STATE, "k-fold sweep before set_train");
  if (!ctx->n_folds) return knn_fail(KNN_ERR_STATE, "k-fold sweep before knn_set_folds");
  if (metric != KNN_METRIC_L2 && metric != KNN_METRIC_L1)
    return knn_fail(KNN_ERR_ARG, "metric must be 0 (L2) or 1 (L1)");
  if ((rc = knn_sweep_check_ks(ks, nk, ctx->train.n - ctx->fold_max, kmax))) return rc;
  return KNN_OK;
}

// Rows [j0, j0 + m) of fold f (positions in the fold's ascending row order, m
// <= kFoldBatch) against the other F - 1 shards, on stream s; the list of K is
// on the device already (sw_ks).  L [nk][m] and idx / dist [m][kmax], flags
// [m] are device buffers of the batch (all required); d_correct / d_conf /
// d_unl (nullable) are ADDED into.  Enqueue only.
static int fold_batch(knn_ctx* ctx, int f, int64_t j0, int64_t m, int32_t nk, int32_t kmax,
                      int32_t metric, int32_t* L, int64_t* d_correct, int64_t* d_idx,
                      double* d_dist, int32_t* d_flags, int64_t* d_conf, int64_t* d_unl,
                      hipStream_t s) {
  int rc;
  const TrainDev& t = ctx->train;
  const int F = ctx->n_folds, parts = F - 1;
  const int64_t first = ctx->fold_off[f] + j0;
  const double* dQ = (const double*)ctx->fold_X.p + first * t.d;  // the queries: no staging copy
  const int32_t* truth = (const int32_t*)ctx->fold_lab.p + first;
  const int32_t* vtruth = d_correct ? truth : nullptr;  // (the votes count only into d_correct)
  const int* dks = (const int*)ctx->sw_ks.p;
  if (kmax == 0) {  // every K is 0: no neighbour is read, every label is -1
    launch_sweep_vote(nullptr, m, 0, t.lab, ctx->idx_off, dks, nk, L, vtruth,
                      (unsigned long long*)d_correct, ctx->cu_count, s);
    launch_fill_i32(d_flags, m, 0, s);
  } else {
    // each shard's exact top w, sorted by (dist, local row), into the packed
    // [parts][m][w] layout; shards below w rows arrive padded (idx -1, dist +inf)
    const int64_t n_rest = t.n - (ctx->fold_off[f + 1] - ctx->fold_off[f]);
    const int w = (int)std::min<int64_t>((int64_t)kmax + 1, n_rest);
    const int64_t PB = packed_part_bytes(m, w);
    if ((rc = ctx->fold_pk.ensure((size_t)(parts * PB)))) return rc;
    if ((rc = ctx->sw_lab.ensure((size_t)m * sizeof(int32_t)))) return rc;
    if (const int64_t sb = merge_scratch_bytes(parts, w, kmax, m))
      if ((rc = ctx->mrg.ensure((size_t)sb))) return rc;
    int p = 0;
    for (int g = 0; g < F; g++) {
      if (g == f) continue;
      knn_ctx* sub = ctx->fold_ctx[g];
      sub->precision = ctx->precision;  // the parent's choices reach every shard
      sub->tune = ctx->tune;
      unsigned char* pb = (unsigned char*)ctx->fold_pk.p + (int64_t)p * PB;
      int64_t* pidx = (int64_t*)(pb + 8 * m * w);
      if ((rc = knn_search_partial_device(sub, dQ, m, w, metric, (double*)pb, pidx,
                                          (int32_t*)(pb + 16 * m * w), s)))
        return rc;
      // local rows -> original rows; rows_of[g] ascends, so the list stays
      // sorted by (dist, idx) and the merge breaks cross-shard ties by train row
      launch_fold_map_idx(pidx, m * w, (const int32_t*)ctx->fold_rowsd.p + ctx->fold_off[g],
                          ctx->fold_off[g + 1] - ctx->fold_off[g], ctx->idx_off, ctx->cu_count, s);
      ctx->last_kmetric = sub->last_kmetric;  // (the last shard search is the call's)
      memcpy(ctx->last_kernel, sub->last_kernel, sizeof ctx->last_kernel);
      p++;
    }
    launch_merge_vote_partials((const double*)ctx->fold_pk.p, nullptr, nullptr, parts, m, w, kmax,
                               (int32_t*)ctx->sw_lab.p, d_idx, d_dist, d_flags, s, 0, m, PB,
                               ctx->mrg.p, MergeTies{});
    // the queries whose label at some K the reference's order among equal
    // distances could change: its std::sort over the n - n_f remaining records
    // in row order is the leave-group-out pass with the fold as the group
    if (ctx->tune.ties) {
      const int64_t per = tie_scratch_bytes(t.n, ctx->class_cnt);
      const int nwg = tie_workgroups(ctx, per);
      if ((rc = ctx->fold_tq.ensure((size_t)m * sizeof(int) + 16))) return rc;
      if ((rc = ctx->fold_qg.ensure((size_t)m * sizeof(int32_t)))) return rc;
      if ((rc = ctx->tie_ws.ensure((size_t)(per * nwg)))) return rc;
      int* tq = (int*)ctx->fold_tq.p + 4;
      int* tcnt = (int*)ctx->fold_tq.p;
      HIP_TRY(hipMemsetAsync(tcnt, 0, sizeof(int), s));
      launch_fill_i32((int32_t*)ctx->fold_qg.p, m, f, s);
      launch_sweep_tie_scan(d_dist, d_idx, d_flags, m, kmax, t.lab, ctx->idx_off, dks, nk,
                            ctx->tune.ties, tq, tcnt, ctx->cu_count, s);
      Sink out{};
      out.mode = MODE_SINGLE;
      out.k = kmax;
      out.idx_off = ctx->idx_off;
      out.labels = (int32_t*)ctx->sw_lab.p;
      out.idx = d_idx;
      out.dist = d_dist;
      out.flags = d_flags;
      out.tie_mode = ctx->tune.ties;
      launch_tie_order_group(metric, t, dQ, tq, tcnt, ctx->class_cnt,
                             (unsigned char*)ctx->tie_ws.p, per, nwg, out,
                             (unsigned long long*)ctx->totals.p + 2, s,
                             (const int32_t*)ctx->fold_qg.p, (const int32_t*)ctx->fold_ids.p);
    }
    sweep_votes(ctx, d_idx, d_dist, m, kmax, dks, nk, L, vtruth, d_correct, s);
  }
  if (d_conf || d_unl)
    launch_eval_confusion(L, nk, m, truth, ctx->class_cnt, (unsigned long long*)d_conf,
                          (unsigned long long*)d_unl, s);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(ctx->done_ev, s));
  ctx->auto_pending = false;  // done_ev now belongs to this call
  return KNN_OK;
}

int knn_kfold_walk(knn_ctx* ctx, int fold0, int step, const int32_t* ks, int32_t nk,
                   int32_t metric, int32_t* out_labels, int64_t* out_correct, int64_t* out_conf,
                   int64_t* out_unl, int64_t* out_idx, double* out_dist, int32_t* out_flags) {
  int rc;
  if ((rc = device_guard(ctx))) return rc;
  int32_t kmax = 0;
  if ((rc = fold_check(ctx, ks, nk, metric, &kmax))) return rc;
  if (fold0 < 0 || step < 1) return knn_fail(KNN_ERR_ARG, "bad fold walk");
  const int64_t n = ctx->train.n;
  const int64_t B = std::min<int64_t>(ctx->fold_max, kFoldBatch);
  const size_t bk = (size_t)B * std::max(kmax, 1);
  const size_t cc = (size_t)ctx->class_cnt * ctx->class_cnt;
  if ((rc = ctx->sw_out.ensure((size_t)B * nk * sizeof(int32_t)))) return rc;
  if ((rc = ctx->sw_corr.ensure((size_t)nk * sizeof(int64_t)))) return rc;
  if ((rc = ctx->ev_conf.ensure((size_t)nk * cc * sizeof(int64_t)))) return rc;
  if ((rc = ctx->ev_unl.ensure((size_t)nk * sizeof(int64_t)))) return rc;
  if ((rc = ctx->o_idx.ensure(bk * sizeof(int64_t)))) return rc;
  if ((rc = ctx->o_dist.ensure(bk * sizeof(double)))) return rc;
  if ((rc = ctx->o_flags.ensure((size_t)B * sizeof(int32_t)))) return rc;
  hipStream_t s = ctx->stream;
  if ((rc = sweep_upload(ctx, ks, nk, (int64_t*)ctx->sw_corr.p, s))) return rc;
  HIP_TRY(hipMemsetAsync(ctx->ev_conf.p, 0, (size_t)nk * cc * sizeof(int64_t), s));
  HIP_TRY(hipMemsetAsync(ctx->ev_unl.p, 0, (size_t)nk * sizeof(int64_t), s));
  // a batch's rows come back in the fold's order and are placed by rows_of
  std::vector<int32_t> hl(out_labels ? (size_t)B * nk : 0), hf(out_flags ? (size_t)B : 0);
  std::vector<int64_t> hi(out_idx ? bk : 0);
  std::vector<double> hd(out_dist ? bk : 0);
  for (int f = fold0; f < ctx->n_folds; f += step) {
    const int64_t nf = ctx->fold_off[f + 1] - ctx->fold_off[f];
    for (int64_t j0 = 0; j0 < nf; j0 += B) {
      const int64_t m = std::min(B, nf - j0);
      rc = fold_batch(ctx, f, j0, m, nk, kmax, metric, (int32_t*)ctx->sw_out.p,
                      out_correct ? (int64_t*)ctx->sw_corr.p : nullptr, (int64_t*)ctx->o_idx.p,
                      (double*)ctx->o_dist.p, (int32_t*)ctx->o_flags.p,
                      out_conf || out_unl ? (int64_t*)ctx->ev_conf.p : nullptr,
                      out_conf || out_unl ? (int64_t*)ctx->ev_unl.p : nullptr, s);
      if (rc) return rc;
      if (!out_labels && !out_flags && !out_idx && !out_dist) continue;
      const size_t mk = (size_t)m * kmax;
      if ((rc = copy_back(hl.data(), ctx->sw_out.p, out_labels ? (size_t)m * nk * 4 : 0, s))) return rc;
      if ((rc = copy_back(hf.data(), ctx->o_flags.p, out_flags ? (size_t)m * 4 : 0, s))) return rc;
      if ((rc = copy_back(hi.data(), ctx->o_idx.p, out_idx ? mk * 8 : 0, s))) return rc;
      if ((rc = copy_back(hd.data(), ctx->o_dist.p, out_dist ? mk * 8 : 0, s))) return rc;
      HIP_TRY(hipStreamSynchronize(s));
      const int32_t* rows = ctx->fold_rows.data() + ctx->fold_off[f] + j0;
      for (int64_t q = 0; q < m; q++) {
        const int64_t r = rows[q];
        if (out_labels)
          for (int32_t j = 0; j < nk; j++) out_labels[(size_t)j * n + r] = hl[(size_t)j * m + q];
        if (out_flags) out_flags[r] = hf[q];
        if (out_idx && kmax) memcpy(out_idx + r * kmax, hi.data() + q * kmax, (size_t)kmax * 8);
        if (out_dist && kmax) memcpy(out_dist + r * kmax, hd.data() + q * kmax, (size_t)kmax * 8);
      }
    }
  }
  if ((rc = copy_back(out_correct, ctx->sw_corr.p, (size_t)nk * sizeof(int64_t), s))) return rc;
  if ((rc = copy_back(out_conf, ctx->ev_conf.p, (size_t)nk * cc * sizeof(int64_t), s))) return rc;
  if ((rc = copy_back(out_unl, ctx->ev_unl.p, (size_t)nk * sizeof(int64_t), s))) return rc;
  HIP_TRY(hipStreamSynchronize(s));
  return KNN_OK;
}

// ---- votes over caller-supplied rows (knn_sweep.hip, knn_eval.hip, knn_wvote.hip)

// knn_vote_sweep_device / knn_vote_sweep_weighted_device up to the launch:
// the argument checks, then the list of K and the zeroed counts on stream s
static int vote_sweep_begin(knn_ctx* ctx, int64_t m, int32_t kmax, const int32_t* ks, int32_t nk,
                            int32_t* d_labels, const int32_t* d_truth, int64_t* d_correct,
                            hipStream_t s) {
  int rc;
  if (m < 0 || m >= (int64_t)INT32_MAX) return knn_fail(KNN_ERR_ARG, "m must be in [0, 2^31)");
  if (kmax < 0) return knn_fail(KNN_ERR_ARG, "kmax must be >= 0");
  int32_t top = 0;
  if ((rc = knn_sweep_check_ks(ks, nk, kmax, &top))) return rc;
  if ((d_truth != nullptr) != (d_correct != nullptr))
    return knn_fail(KNN_ERR_ARG, "d_truth and d_correct go together (both or neither)");
  if (!d_labels) return knn_fail(KNN_ERR_ARG, "null labels output");
  return sweep_upload(ctx, ks, nk, d_correct, s);
}

// knn_vote_counts_device / knn_vote_weights_device: the geometry of one vote
// over the first k entries of rows [m][kmax], and the output `what`
static int check_vote_args(int64_t m, int32_t kmax, int32_t k, int32_t class_cnt, const void* out,
                           const char* what) {
  if (m < 0 || m >= (int64_t)INT32_MAX) return knn_fail(KNN_ERR_ARG, "m must be in [0, 2^31)");
  if (kmax < 0) return knn_fail(KNN_ERR_ARG, "kmax must be >= 0");
  if (k < 0) return knn_fail(KNN_ERR_ARG, "k must be >= 0");
  if (k > kmax)
    return knn_fail(KNN_ERR_ARG, "k = " + std::to_string(k) + " exceeds kmax = " +
                                     std::to_string(kmax) + " (the entries of a row)");
  if (class_cnt <= 0) return knn_fail(KNN_ERR_ARG, "class_cnt must be > 0");
  if (!out) return knn_fail(KNN_ERR_ARG, std::string("null ") + what);
  return KNN_OK;
}

extern "C" {

int knn_classify_device(knn_ctx* ctx, const double* dQ, int64_t m, int32_t k, int32_t metric,
                        int32_t* d_labels, int64_t* d_idx, double* d_dist, int32_t* d_flags,
                        void* stream) {
  int rc;
  if ((rc = device_guard(ctx))) return rc;
  if ((rc = check_query_args(ctx, m, k, metric))) return rc;
  if (!d_labels) return knn_fail(KNN_ERR_ARG, "null labels output");
  hipStream_t s = stream_of(ctx, stream);
  if (m == 0) return KNN_OK;
  if (!dQ) return knn_fail(KNN_ERR_ARG, "null query pointer");
  if (k == 0) {  // cpp:324: max_label stays -1
    launch_fill_i32(d_labels, m, -1, s);
    if (d_flags) launch_fill_i32(d_flags, m, 0, s);
    HIP_TRY(hipGetLastError());
    return KNN_OK;
  }
  Sink sink{};
  sink.mode = MODE_SINGLE;
  sink.k = k;
  sink.idx_off = ctx->idx_off;
  sink.labels = d_labels;
  sink.idx = d_idx;
  sink.dist = d_dist;
  sink.flags = d_flags;
  const int W = (int)std::min<int64_t>((int64_t)k + 1, ctx->train.n);
  if (ctx->vote == KNN_VOTE_DISTANCE) {
    // the search and its tie pass as in uniform mode, into internal rows where
    // the caller passes none; then the weighted vote over those rows replaces
    // the labels (a one-entry list of K)
    if (!d_idx && (rc = ctx->sw_idx.ensure((size_t)m * k * sizeof(int64_t)))) return rc;
    if (!d_dist && (rc = ctx->sw_dist.ensure((size_t)m * k * sizeof(double)))) return rc;
    if ((rc = ctx->sw_ks.ensure(sizeof(int32_t)))) return rc;
    if (!d_idx) sink.idx = (int64_t*)ctx->sw_idx.p;
    if (!d_dist) sink.dist = (double*)ctx->sw_dist.p;
    rc = k > kMaxK ? run_large_k(ctx, dQ, m, W, metric, sink, s)
                   : knn_run_search(ctx, dQ, m, W, metric, sink, s);
    if (rc) return rc;
    launch_fill_i32((int32_t*)ctx->sw_ks.p, 1, k, s);
    launch_wvote_sweep(sink.idx, sink.dist, m, k, ctx->train.lab, ctx->idx_off,
                       (const int*)ctx->sw_ks.p, 1, d_labels, nullptr, nullptr, ctx->cu_count, s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ctx->done_ev, s));  // the call ends after the vote
    return KNN_OK;
  }
  if (k > kMaxK) return run_large_k(ctx, dQ, m, W, metric, sink, s);
  return knn_run_search(ctx, dQ, m, W, metric, sink, s);
}

int knn_classify(knn_ctx* ctx, const double* Q, int64_t m, int32_t k, int32_t metric,
                 int32_t* out_labels, int64_t* out_idx, double* out_dist, int32_t* out_flags) {
  int rc;
  if ((rc = device_guard(ctx))) return rc;
  if ((rc = check_query_args(ctx, m, k, metric))) return rc;
  if (!out_labels) return knn_fail(KNN_ERR_ARG, "null labels output");
  if (m == 0) return KNN_OK;
  if (!Q) return knn_fail(KNN_ERR_ARG, "null query pointer");
  const int d = ctx->train.d;
  if ((rc = ctx->Q64.ensure((size_t)m * d * sizeof(double)))) return rc;
  if ((rc = ctx->o_lab.ensure((size_t)m * sizeof(int32_t)))) return rc;
  if ((rc = ctx->o_flags.ensure((size_t)m * sizeof(int32_t)))) return rc;
  if (out_idx && (rc = ctx->o_idx.ensure((size_t)m * std::max(k, 1) * sizeof(int64_t)))) return rc;
  if (out_dist && (rc = ctx->o_dist.ensure((size_t)m * std::max(k, 1) * sizeof(double)))) return rc;
  hipStream_t s = ctx->stream;
  HIP_TRY(hipMemcpyAsync(ctx->Q64.p, Q, (size_t)m * d * sizeof(double), hipMemcpyHostToDevice, s));
  rc = knn_classify_device(ctx, (const double*)ctx->Q64.p, m, k, metric, (int32_t*)ctx->o_lab.p,
                           out_idx ? (int64_t*)ctx->o_idx.p : nullptr,
                           out_dist ? (double*)ctx->o_dist.p : nullptr,
                           (int32_t*)ctx->o_flags.p, s);
  if (rc) return rc;
  if ((rc = copy_back(out_labels, ctx->o_lab.p, (size_t)m * sizeof(int32_t), s))) return rc;
  if ((rc = copy_back(out_flags, ctx->o_flags.p, (size_t)m * sizeof(int32_t), s))) return rc;
  if ((rc = copy_back(out_idx, ctx->o_idx.p, (size_t)m * k * sizeof(int64_t), s))) return rc;
  if ((rc = copy_back(out_dist, ctx->o_dist.p, (size_t)m * k * sizeof(double), s))) return rc;
  HIP_TRY(hipStreamSynchronize(s));
  return KNN_OK;
}

int knn_vote_sweep_device(knn_ctx* ctx, const int64_t* d_idx, int64_t m, int32_t kmax,
                          const int32_t* d_lab, int64_t idx_base, const int32_t* ks, int32_t nk,
                          int32_t* d_labels, const int32_t* d_truth, int64_t* d_correct,
                          void* stream) {
  int rc;
  if ((rc = device_guard(ctx))) return rc;
  hipStream_t s = stream_of(ctx, stream);
  if ((rc = vote_sweep_begin(ctx, m, kmax, ks, nk, d_labels, d_truth, d_correct, s))) return rc;
  if (m == 0) return KNN_OK;
  if (kmax > 0 && (!d_idx || !d_lab)) return knn_fail(KNN_ERR_ARG, "null neighbour rows / labels");
  launch_sweep_vote(d_idx, m, kmax, d_lab, idx_base, (const int*)ctx->sw_ks.p, nk, d_labels,
                    d_truth, (unsigned long long*)d_correct, ctx->cu_count, s);
  HIP_TRY(hipGetLastError());
  return KNN_OK;
}

int knn_classify_sweep_device(knn_ctx* ctx, const double* dQ, int64_t m, const int32_t* ks,
                              int32_t nk, int32_t metric, int32_t* d_labels,
                              const int32_t* d_truth, int64_t* d_correct, int64_t* d_idx,
                              double* d_dist, int32_t* d_flags, void* stream) {
  int rc;
  if ((rc = device_guard(ctx))) return rc;
  return sweep_run(ctx, dQ, m, Excl{}, ks, nk, metric, d_labels, d_truth, d_correct, d_idx,
                   d_dist, d_flags, stream_of(ctx, stream));
}

int knn_classify_sweep(knn_ctx* ctx, const double* Q, int64_t m, const int32_t* ks, int32_t nk,
                       int32_t metric, int32_t* out_labels, const int32_t* truth,
                       int64_t* out_correct, int64_t* out_idx, double* out_dist,
                       int32_t* out_flags) {
  int rc;
  if ((rc = device_guard(ctx))) return rc;
  if ((rc = check_query_args(ctx, m, 0, metric))) return rc;
  int32_t kmax = 0;
  if ((rc = knn_sweep_check_ks(ks, nk, ctx->train.n, &kmax))) return rc;
  if ((truth != nullptr) != (out_correct != nullptr))
    return knn_fail(KNN_ERR_ARG, "truth and out_correct go together (both or neither)");
  if (!out_labels) return knn_fail(KNN_ERR_ARG, "null labels output");
  if (m > 0 && !Q) return knn_fail(KNN_ERR_ARG, "null query pointer");
  return host_sweep(ctx, Q, m, ks, nk, kmax, metric, false, out_labels, truth, out_correct,
                    nullptr, nullptr, out_idx, out_dist, out_flags);
}

// ---- K sweep under exclusion / leave-one-out (knn_loo.hip, cpp:308-343 with
// the train set as its own validation set)

int knn_classify_sweep_excl_device(knn_ctx* ctx, const double* dQ, int64_t m,
                                   const int64_t* d_excl, const int32_t* ks, int32_t nk,
                                   int32_t metric, int32_t* d_labels, const int32_t* d_truth,
                                   int64_t* d_correct, int64_t* d_idx, double* d_dist,
                                   int32_t* d_flags, void* stream) {
  int rc;
  if ((rc = device_guard(ctx))) return rc;
  return sweep_run(ctx, dQ, m, Excl::of_row(d_excl), ks, nk, metric, d_labels, d_truth,
                   d_correct, d_idx, d_dist, d_flags, stream_of(ctx, stream));
}

int knn_loo_sweep_device(knn_ctx* ctx, int64_t row0, int64_t rows, const int32_t* ks, int32_t nk,
                         int32_t metric, int32_t* d_labels, int64_t* d_correct, int64_t* d_idx,
                         double* d_dist, int32_t* d_flags, void* stream) {
  int rc;
  if ((rc = device_guard(ctx))) return rc;
  if (!d_labels) return knn_fail(KNN_ERR_ARG, "null labels output");
  return knn_sweep_rows(ctx, row0, rows, false, ks, nk, metric, d_labels, d_correct, d_idx, d_dist,
                        d_flags, nullptr, nullptr, true, stream_of(ctx, stream));
}

int knn_loo_sweep(knn_ctx* ctx, const int32_t* ks, int32_t nk, int32_t metric, int32_t* out_labels,
                  int64_t* out_correct, int64_t* out_idx, double* out_dist, int32_t* out_flags) {
  int rc;
  if ((rc = device_guard(ctx))) return rc;
  if ((rc = check_query_args(ctx, 0, 0, metric))) return rc;
  int32_t kmax = 0;
  if ((rc = knn_sweep_check_ks(ks, nk, ctx->train.n - 1, &kmax))) return rc;
  if (!out_labels) return knn_fail(KNN_ERR_ARG, "null labels output");
  return host_rows_walk(ctx, false, ks, nk, kmax, metric, out_labels, out_correct, nullptr,
                        nullptr, out_idx, out_dist, out_flags);
}


// ---- K sweep under group exclusion / leave-group-out (knn_lgo.hip)

// attaches device-resident group ids to the current train set: the range
// check and the group-size histogram run on the device, the call waits for
// {first bad row, gmax} as set_train waits for its checks
static int attach_groups(knn_ctx* ctx, const int32_t* d_groups, int32_t n_groups) {
  int rc;
  const int64_t n = ctx->train.n;
  ctx->groups = nullptr;
  ctx->n_groups = ctx->gmax = 0;
  if (n_groups <= 0) return knn_fail(KNN_ERR_ARG, "n_groups must be > 0");
  if ((rc = ctx->grp_hist.ensure((size_t)n_groups * sizeof(int32_t)))) return rc;
  if ((rc = ctx->grp_stat.ensure(2 * sizeof(unsigned long long)))) return rc;
  hipStream_t s = ctx->stream;
  unsigned long long h[2] = {(unsigned long long)n, 0};  // first bad row (n: none) | gmax
  HIP_TRY(hipMemsetAsync(ctx->grp_hist.p, 0, (size_t)n_groups * sizeof(int32_t), s));
  HIP_TRY(hipMemcpyAsync(ctx->grp_stat.p, h, sizeof(h), hipMemcpyHostToDevice, s));
  launch_lgo_group_stats(d_groups, n, n_groups, (int32_t*)ctx->grp_hist.p,
                         (unsigned long long*)ctx->grp_stat.p,
                         (int32_t*)((unsigned long long*)ctx->grp_stat.p + 1), ctx->cu_count, s);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(h, ctx->grp_stat.p, sizeof(h), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (h[0] < (unsigned long long)n)
    return knn_fail(KNN_ERR_ARG, "group id out of [0, n_groups) at row " + std::to_string(h[0]));
  ctx->groups = d_groups;
  ctx->n_groups = n_groups;
  ctx->gmax = (int32_t)(h[1] & 0xffffffffu);
  return KNN_OK;
}

int knn_set_groups_device(knn_ctx* ctx, const int32_t* d_groups, int32_t n_groups) {
  int rc;
  if ((rc = device_guard(ctx))) return rc;
  if (!ctx->trained) return knn_fail(KNN_ERR_STATE, "set_groups before set_train");
  if (!d_groups) {  // clears the groups
    ctx->groups = nullptr;
    ctx->n_groups = ctx->gmax = 0;
    return KNN_OK;
  }
  return attach_groups(ctx, d_groups, n_groups);
}

int knn_set_groups(knn_ctx* ctx, const int32_t* groups, int32_t n_groups) {
  int rc;
  if ((rc = device_guard(ctx))) return rc;
  if (!ctx->trained) return knn_fail(KNN_ERR_STATE, "set_groups before set_train");
  if (!groups) return knn_set_groups_device(ctx, nullptr, 0);
  const int64_t n = ctx->train.n;
  ctx->groups = nullptr;  // (the copy below overwrites the ids the last call attached)
  ctx->n_groups = ctx->gmax = 0;
  if ((rc = ctx->grp_own.ensure((size_t)n * sizeof(int32_t)))) return rc;
  HIP_TRY(hipMemcpyAsync(ctx->grp_own.p, groups, (size_t)n * sizeof(int32_t),
                         hipMemcpyHostToDevice, ctx->stream));
  return attach_groups(ctx, (const int32_t*)ctx->grp_own.p, n_groups);
}

int32_t knn_get_group_max(knn_ctx* ctx) { return ctx && ctx->groups ? ctx->gmax : 0; }

int knn_classify_sweep_gexcl_device(knn_ctx* ctx, const double* dQ, int64_t m,
                                    const int32_t* d_qgroup, const int32_t* ks, int32_t nk,
                                    int32_t metric, int32_t* d_labels, const int32_t* d_truth,
                                    int64_t* d_correct, int64_t* d_idx, double* d_dist,
                                    int32_t* d_flags, void* on_stream) {
  int rc;
  if ((rc = device_guard(ctx))) return rc;
  return sweep_run(ctx, dQ, m, Excl::of_group(d_qgroup), ks, nk, metric, d_labels, d_truth,
                   d_correct, d_idx, d_dist, d_flags, stream_of(ctx, on_stream));
}

int knn_lgo_sweep_device(knn_ctx* ctx, int64_t row0, int64_t rows, const int32_t* ks, int32_t nk,
                         int32_t metric, int32_t* d_labels, int64_t* d_correct, int64_t* d_idx,
                         double* d_dist, int32_t* d_flags, void* on_stream) {
  int rc;
  if ((rc = device_guard(ctx))) return rc;
  if (!d_labels) return knn_fail(KNN_ERR_ARG, "null labels output");
  return knn_sweep_rows(ctx, row0, rows, true, ks, nk, metric, d_labels, d_correct, d_idx, d_dist,
                        d_flags, nullptr, nullptr, true, stream_of(ctx, on_stream));
}

int knn_lgo_sweep(knn_ctx* ctx, const int32_t* ks, int32_t nk, int32_t metric, int32_t* out_labels,
                  int64_t* out_correct, int64_t* out_conf, int64_t* out_unl, int64_t* out_idx,
                  double* out_dist, int32_t* out_flags) {
  int rc;
  if ((rc = device_guard(ctx))) return rc;
  if ((rc = check_query_args(ctx, 0, 0, metric))) return rc;
  if (!ctx->groups) return knn_fail(KNN_ERR_STATE, "leave-group-out sweep before knn_set_groups");
  int32_t kmax = 0;
  if ((rc = knn_sweep_check_ks(ks, nk, ctx->train.n - ctx->gmax, &kmax))) return rc;
  if (!out_labels && !out_conf) return knn_fail(KNN_ERR_ARG, "null labels output");
  return host_rows_walk(ctx, true, ks, nk, kmax, metric, out_labels, out_correct, out_conf,
                        out_unl, out_idx, out_dist, out_flags);
}


// ---- F-fold cross-validated K sweep on fold shards (knn_fold.hip)

int knn_set_folds(knn_ctx* ctx, const int32_t* folds, int32_t n_folds) {
  int rc;
  if ((rc = device_guard(ctx))) return rc;
  if (!ctx->trained) return knn_fail(KNN_ERR_STATE, "set_folds before set_train");
  if (ctx->n_folds) {  // (work of the last folds may still run on a caller's stream)
    HIP_TRY(hipDeviceSynchronize());
    fold_clear(ctx);
  }
  if (!folds) return KNN_OK;  // clears the folds
  if (n_folds < 2 || n_folds > kMaxParts)
    return knn_fail(KNN_ERR_ARG, "n_folds = " + std::to_string(n_folds) + " must be in [2, 64]");
  const TrainDev& t = ctx->train;
  const int64_t n = t.n;
  const int d = t.d;
  // the range check and the fold sizes: set_groups' kernel
  if ((rc = ctx->fold_ids.ensure((size_t)n * sizeof(int32_t)))) return rc;
  if ((rc = ctx->grp_hist.ensure((size_t)n_folds * sizeof(int32_t)))) return rc;
  if ((rc = ctx->grp_stat.ensure(2 * sizeof(unsigned long long)))) return rc;
  hipStream_t s = ctx->stream;
  unsigned long long h[2] = {(unsigned long long)n, 0};  // first bad row (n: none) | largest fold
  std::vector<int32_t> hist((size_t)n_folds, 0);
  HIP_TRY(hipMemcpyAsync(ctx->fold_ids.p, folds, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemsetAsync(ctx->grp_hist.p, 0, (size_t)n_folds * sizeof(int32_t), s));
  HIP_TRY(hipMemcpyAsync(ctx->grp_stat.p, h, sizeof(h), hipMemcpyHostToDevice, s));
  launch_lgo_group_stats((const int32_t*)ctx->fold_ids.p, n, n_folds, (int32_t*)ctx->grp_hist.p,
                         (unsigned long long*)ctx->grp_stat.p,
                         (int32_t*)((unsigned long long*)ctx->grp_stat.p + 1), ctx->cu_count, s);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(h, ctx->grp_stat.p, sizeof(h), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(hist.data(), ctx->grp_hist.p, (size_t)n_folds * sizeof(int32_t),
                         hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (h[0] < (unsigned long long)n)
    return knn_fail(KNN_ERR_ARG, "fold id out of [0, n_folds) at row " + std::to_string(h[0]));
  for (int f = 0; f < n_folds; f++)
    if (hist[f] <= 0) return knn_fail(KNN_ERR_ARG, "fold " + std::to_string(f) + " is empty");
  // rows_of: the stable fold-major order (inside a fold the rows ascend)
  std::vector<int64_t> off((size_t)n_folds + 1, 0);
  for (int f = 0; f < n_folds; f++) off[f + 1] = off[f] + hist[f];
  std::vector<int32_t> rows((size_t)n);
  {
    std::vector<int64_t> at(off.begin(), off.end() - 1);
    for (int64_t r = 0; r < n; r++) rows[(size_t)at[folds[r]]++] = (int32_t)r;
  }
  if ((rc = ctx->fold_rowsd.ensure((size_t)n * sizeof(int32_t)))) return rc;
  if ((rc = ctx->fold_X.ensure((size_t)n * d * sizeof(double)))) return rc;
  if ((rc = ctx->fold_lab.ensure((size_t)n * sizeof(int32_t)))) return rc;
  HIP_TRY(hipMemcpyAsync(ctx->fold_rowsd.p, rows.data(), (size_t)n * sizeof(int32_t),
                         hipMemcpyHostToDevice, s));
  launch_fold_gather(t.X64, t.lab, (const int32_t*)ctx->fold_rowsd.p, n, d, (double*)ctx->fold_X.p,
                     (int32_t*)ctx->fold_lab.p, ctx->cu_count, s);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(s));
  // one sub-context per fold over its (borrowed) slice, local indices from 0;
  // precision and tuning are the parent's, the vote stays with the parent
  for (int f = 0; f < n_folds; f++) {
    knn_ctx* sub = nullptr;
    if ((rc = knn_create(&sub, ctx->device))) break;
    ctx->fold_ctx.push_back(sub);
    sub->precision = ctx->precision;
    sub->tune = ctx->tune;
    if ((rc = knn_set_train_device(sub, (const double*)ctx->fold_X.p + off[f] * d,
                                   (const int32_t*)ctx->fold_lab.p + off[f], hist[f], d,
                                   ctx->class_cnt, 0)))
      break;
  }
  if (rc) {
    const std::string msg = knn_last_error();
    fold_clear(ctx);
    return knn_fail(rc, "fold shard: " + msg);
  }
  ctx->fold_off = std::move(off);
  ctx->fold_rows = std::move(rows);
  ctx->n_folds = n_folds;
  ctx->fold_max = (int32_t)(h[1] & 0xffffffffu);
  return KNN_OK;
}

int32_t knn_get_fold_max(knn_ctx* ctx) { return ctx ? ctx->fold_max : 0; }

int knn_kfold_sweep_device(knn_ctx* ctx, int32_t fold, const int32_t* ks, int32_t nk,
                           int32_t metric, int32_t* d_labels, int64_t* d_correct, int64_t* d_idx,
                           double* d_dist, int32_t* d_flags, void* on_stream) {
  int rc;
  if ((rc = device_guard(ctx))) return rc;
  int32_t kmax = 0;
  if ((rc = fold_check(ctx, ks, nk, metric, &kmax))) return rc;
  if (fold < 0 || fold >= ctx->n_folds)
    return knn_fail(KNN_ERR_ARG, "fold = " + std::to_string(fold) + " outside [0, " +
                                     std::to_string(ctx->n_folds) + ")");
  if (!d_labels) return knn_fail(KNN_ERR_ARG, "null labels output");
  hipStream_t s = stream_of(ctx, on_stream);
  const int64_t nf = ctx->fold_off[fold + 1] - ctx->fold_off[fold];
  const int64_t B = std::min<int64_t>(nf, kFoldBatch);
  const size_t bk = (size_t)B * std::max(kmax, 1);
  if (nf > B && (rc = ctx->sw_out.ensure((size_t)B * nk * sizeof(int32_t)))) return rc;
  if (!d_idx && (rc = ctx->o_idx.ensure(bk * sizeof(int64_t)))) return rc;
  if (!d_dist && (rc = ctx->o_dist.ensure(bk * sizeof(double)))) return rc;
  if (!d_flags && (rc = ctx->o_flags.ensure((size_t)B * sizeof(int32_t)))) return rc;
  if ((rc = sweep_upload(ctx, ks, nk, d_correct, s))) return rc;
  for (int64_t j0 = 0; j0 < nf; j0 += B) {
    const int64_t m = std::min(B, nf - j0);
    // one batch writes the caller's [nk][nf] rows itself; several go through
    // the workspace, each into its columns
    int32_t* L = nf > B ? (int32_t*)ctx->sw_out.p : d_labels;
    rc = fold_batch(ctx, fold, j0, m, nk, kmax, metric, L, d_correct,
                    d_idx ? d_idx + j0 * kmax : (int64_t*)ctx->o_idx.p,
                    d_dist ? d_dist + j0 * kmax : (double*)ctx->o_dist.p,
                    d_flags ? d_flags + j0 : (int32_t*)ctx->o_flags.p, nullptr, nullptr, s);
    if (rc) return rc;
    if (nf > B)
      HIP_TRY(hipMemcpy2DAsync(d_labels + j0, (size_t)nf * sizeof(int32_t), L,
                               (size_t)m * sizeof(int32_t), (size_t)m * sizeof(int32_t),
                               (size_t)nk, hipMemcpyDeviceToDevice, s));
  }
  return KNN_OK;
}

int knn_kfold_sweep(knn_ctx* ctx, const int32_t* ks, int32_t nk, int32_t metric,
                    int32_t* out_labels, int64_t* out_correct, int64_t* out_conf, int64_t* out_unl,
                    int64_t* out_idx, double* out_dist, int32_t* out_flags) {
  int rc;
  if ((rc = device_guard(ctx))) return rc;
  int32_t kmax = 0;
  if ((rc = fold_check(ctx, ks, nk, metric, &kmax))) return rc;
  if (!out_labels && !out_conf) return knn_fail(KNN_ERR_ARG, "null labels output");
  return knn_kfold_walk(ctx, 0, 1, ks, nk, metric, out_labels, out_correct, out_conf, out_unl,
                        out_idx, out_dist, out_flags);
}


// ---- per-class evaluation (knn_eval.hip): the confusion matrix at every K
// of a sweep, the vote counts of ordered neighbour rows

int knn_confusion_device(knn_ctx* ctx, const int32_t* d_labels, int32_t nk, int64_t m,
                         const int32_t* d_truth, int32_t class_cnt, int64_t* d_conf,
                         int64_t* d_unl, void* stream) {
  int rc;
  if ((rc = device_guard(ctx))) return rc;
  if (nk < 1 || nk > 4096)
    return knn_fail(KNN_ERR_ARG, "nk = " + std::to_string(nk) + " must be in [1, 4096]");
  if (m < 0 || m >= (int64_t)INT32_MAX) return knn_fail(KNN_ERR_ARG, "m must be in [0, 2^31)");
  if (class_cnt <= 0) return knn_fail(KNN_ERR_ARG, "class_cnt must be > 0");
  if (!d_conf) return knn_fail(KNN_ERR_ARG, "null d_conf");
  if (m == 0) return KNN_OK;
  if (!d_truth) return knn_fail(KNN_ERR_ARG, "null d_truth");
  if (!d_labels) return knn_fail(KNN_ERR_ARG, "null d_labels");
  hipStream_t s = stream_of(ctx, stream);
  launch_eval_confusion(d_labels, nk, m, d_truth, class_cnt, (unsigned long long*)d_conf,
                        (unsigned long long*)d_unl, s);
  HIP_TRY(hipGetLastError());
  return KNN_OK;
}

int knn_vote_counts_device(knn_ctx* ctx, const int64_t* d_idx, int64_t m, int32_t kmax,
                           const int32_t* d_lab, int64_t idx_base, int32_t k, int32_t class_cnt,
                           int32_t* d_counts, void* stream) {
  int rc;
  if ((rc = device_guard(ctx))) return rc;
  if ((rc = check_vote_args(m, kmax, k, class_cnt, d_counts, "d_counts"))) return rc;
  if (m == 0) return KNN_OK;
  if (k > 0 && (!d_idx || !d_lab)) return knn_fail(KNN_ERR_ARG, "null neighbour rows / labels");
  HIP_TRY(launch_eval_vote_counts(d_idx, m, kmax, d_lab, idx_base, k, class_cnt, d_counts,
                                  ctx->cu_count, stream_of(ctx, stream)));
  HIP_TRY(hipGetLastError());
  return KNN_OK;
}

// ---- distance-weighted voting over caller-supplied rows (knn_wvote.hip)

int knn_vote_sweep_weighted_device(knn_ctx* ctx, const int64_t* d_idx, const double* d_dist,
                                   int64_t m, int32_t kmax, const int32_t* d_lab,
                                   int64_t idx_base, const int32_t* ks, int32_t nk,
                                   int32_t* d_labels, const int32_t* d_truth, int64_t* d_correct,
                                   void* stream) {
  int rc;
  if ((rc = device_guard(ctx))) return rc;
  hipStream_t s = stream_of(ctx, stream);
  if ((rc = vote_sweep_begin(ctx, m, kmax, ks, nk, d_labels, d_truth, d_correct, s))) return rc;
  if (m == 0) return KNN_OK;
  if (kmax > 0 && (!d_idx || !d_dist || !d_lab))
    return knn_fail(KNN_ERR_ARG, "null neighbour rows / distances / labels");
  launch_wvote_sweep(d_idx, d_dist, m, kmax, d_lab, idx_base, (const int*)ctx->sw_ks.p, nk,
                     d_labels, d_truth, (unsigned long long*)d_correct, ctx->cu_count, s);
  HIP_TRY(hipGetLastError());
  return KNN_OK;
}

int knn_vote_weights_device(knn_ctx* ctx, const int64_t* d_idx, const double* d_dist, int64_t m,
                            int32_t kmax, const int32_t* d_lab, int64_t idx_base, int32_t k,
                            int32_t class_cnt, double* d_wsum, void* stream) {
  int rc;
  if ((rc = device_guard(ctx))) return rc;
  if ((rc = check_vote_args(m, kmax, k, class_cnt, d_wsum, "d_wsum"))) return rc;
  if (m == 0) return KNN_OK;
  if (k > 0 && (!d_idx || !d_dist || !d_lab))
    return knn_fail(KNN_ERR_ARG, "null neighbour rows / distances / labels");
  launch_wvote_sums(d_idx, d_dist, m, kmax, d_lab, idx_base, k, class_cnt, d_wsum,
                    ctx->cu_count, stream_of(ctx, stream));
  HIP_TRY(hipGetLastError());
  return KNN_OK;
}

int knn_classify_sweep_eval_device(knn_ctx* ctx, const double* dQ, int64_t m,
                                   const int64_t* d_excl, const int32_t* ks, int32_t nk,
                                   int32_t metric, int32_t* d_labels, const int32_t* d_truth,
                                   int64_t* d_correct, int64_t* d_conf, int64_t* d_unl,
                                   void* stream) {
  int rc;
  if ((rc = device_guard(ctx))) return rc;
  return sweep_eval(ctx, dQ, m, d_excl, ks, nk, metric, d_labels, d_truth, d_correct, d_conf,
                    d_unl, stream_of(ctx, stream));
}

int knn_loo_sweep_eval_device(knn_ctx* ctx, int64_t row0, int64_t rows, const int32_t* ks,
                              int32_t nk, int32_t metric, int32_t* d_labels, int64_t* d_correct,
                              int64_t* d_conf, int64_t* d_unl, void* stream) {
  int rc;
  if ((rc = device_guard(ctx))) return rc;
  return knn_sweep_rows(ctx, row0, rows, false, ks, nk, metric, d_labels, d_correct, nullptr,
                        nullptr, nullptr, d_conf, d_unl, true, stream_of(ctx, stream));
}

int knn_classify_sweep_eval(knn_ctx* ctx, const double* Q, int64_t m, const int32_t* ks,
                            int32_t nk, int32_t metric, int32_t* out_labels, const int32_t* truth,
                            int64_t* out_correct, int64_t* out_conf, int64_t* out_unl) {
  int rc;
  if ((rc = device_guard(ctx))) return rc;
  if ((rc = check_query_args(ctx, m, 0, metric))) return rc;
  int32_t kmax = 0;
  if ((rc = knn_sweep_check_ks(ks, nk, ctx->train.n, &kmax))) return rc;
  if (!truth) return knn_fail(KNN_ERR_ARG, "null truth (the evaluation needs the true labels)");
  if (m > 0 && !Q) return knn_fail(KNN_ERR_ARG, "null query pointer");
  return host_sweep(ctx, Q, m, ks, nk, kmax, metric, true, out_labels, truth, out_correct,
                    out_conf, out_unl, nullptr, nullptr, nullptr);
}

int knn_loo_sweep_eval(knn_ctx* ctx, const int32_t* ks, int32_t nk, int32_t metric,
                       int32_t* out_labels, int64_t* out_correct, int64_t* out_conf,
                       int64_t* out_unl) {
  int rc;
  if ((rc = device_guard(ctx))) return rc;
  if ((rc = check_query_args(ctx, 0, 0, metric))) return rc;
  int32_t kmax = 0;
  if ((rc = knn_sweep_check_ks(ks, nk, ctx->train.n - 1, &kmax))) return rc;
  return host_rows_walk(ctx, false, ks, nk, kmax, metric, out_labels, out_correct, out_conf,
                        out_unl, nullptr, nullptr, nullptr);
}


int knn_search_partial_device(knn_ctx* ctx, const double* dQ, int64_t m, int32_t w,
                              int32_t metric, double* d_dist, int64_t* d_idx, int32_t* d_lab,
                              void* stream) {
  int rc;
  if ((rc = device_guard(ctx))) return rc;
  if (!ctx->trained) return knn_fail(KNN_ERR_STATE, "search before set_train");
  if (w <= 0) return knn_fail(KNN_ERR_ARG, "w must be >= 1");
  if (metric != KNN_METRIC_L2 && metric != KNN_METRIC_L1)
    return knn_fail(KNN_ERR_ARG, "metric must be 0 (L2) or 1 (L1)");
  if (m < 0 || m >= (int64_t)INT32_MAX) return knn_fail(KNN_ERR_ARG, "bad m");
  if (!d_dist || !d_idx || !d_lab) return knn_fail(KNN_ERR_ARG, "null output");
  if (m == 0) return KNN_OK;
  hipStream_t s = stream_of(ctx, stream);
  Sink sink{};
  sink.mode = MODE_PARTIAL;
  sink.w = w;
  sink.idx_off = ctx->idx_off;
  sink.idx = d_idx;
  sink.dist = d_dist;
  sink.plab = d_lab;
  // a shard smaller than w yields min(w, n) entries; the tail is padded
  const int W = (int)std::min<int64_t>(w, ctx->train.n);
  if (w > kMaxK + 1) return run_large_k(ctx, dQ, m, W, metric, sink, s);
  return knn_run_search(ctx, dQ, m, W, metric, sink, s);
}

int knn_merge_vote_device(knn_ctx* ctx, const double* d_dist, const int64_t* d_idx,
                          const int32_t* d_lab, int32_t parts, int64_t m, int32_t w, int32_t k,
                          int64_t q0, int64_t mq, int32_t* d_labels, int64_t* d_out_idx,
                          double* d_out_dist, int32_t* d_flags, void* stream) {
  int rc;
  if ((rc = device_guard(ctx))) return rc;
  if (parts <= 0 || w <= 0 || k < 0 || k > w || (int64_t)parts * w >= INT32_MAX)
    return knn_fail(KNN_ERR_ARG, "bad merge geometry (need 0 <= k <= w)");
  if (q0 < 0 || mq < 0 || q0 + mq > m) return knn_fail(KNN_ERR_ARG, "query slice out of range");
  if (!d_labels) return knn_fail(KNN_ERR_ARG, "null labels output");
  if (mq == 0) return KNN_OK;
  hipStream_t s = stream_of(ctx, stream);
  // unions beyond the LDS kernel's 4096 entries: rank merge through scratch
  if (const int64_t sb = merge_scratch_bytes(parts, w, k, mq))
    if ((rc = ctx->mrg.ensure((size_t)sb))) return rc;
  MergeTies mt;
  mt.mode = ctx->tune.ties;
  launch_merge_vote_partials(d_dist, d_idx, d_lab, parts, m, w, k, d_labels, d_out_idx,
                             d_out_dist, d_flags, s, q0, mq, 0, ctx->mrg.p, mt);
  HIP_TRY(hipGetLastError());
  return KNN_OK;
}

int knn_shard_distances_device(knn_ctx* ctx, const double* dQ, const int32_t* d_qsel,
                               int32_t nsel, int32_t metric, double* d_out, void* stream) {
  int rc;
  if ((rc = device_guard(ctx))) return rc;
  if (!ctx->trained) return knn_fail(KNN_ERR_STATE, "shard distances before set_train");
  if (nsel < 0 || metric < 0 || metric > 1) return knn_fail(KNN_ERR_ARG, "bad shard distance arguments");
  if (nsel == 0) return KNN_OK;
  if (!dQ || !d_out) return knn_fail(KNN_ERR_ARG, "null pointer");
  hipStream_t s = stream_of(ctx, stream);
  launch_shard_dist(metric, ctx->train, dQ, d_qsel, nsel, d_out, s);
  HIP_TRY(hipGetLastError());
  return KNN_OK;
}

int knn_tie_resolve_device(knn_ctx* ctx, const double* d_D, int32_t parts, const int64_t* rows,
                           int32_t nsel, const int32_t* d_lab_all, const int32_t* d_orow,
                           int32_t k, int32_t* d_labels, int64_t* d_idx, double* d_dist,
                           int32_t* d_flags, void* stream) {
  int rc;
  if ((rc = device_guard(ctx))) return rc;
  if (!ctx->trained) return knn_fail(KNN_ERR_STATE, "tie resolve before set_train");
  if (parts <= 0 || parts > kMaxParts || nsel < 0 || !rows)
    return knn_fail(KNN_ERR_ARG, "bad tie resolve geometry (1 <= parts <= 64)");
  PartRows pr{};
  pr.parts = parts;
  for (int p = 0; p < parts; p++) {
    if (rows[p] < 0) return knn_fail(KNN_ERR_ARG, "negative part rows");
    pr.off[p + 1] = pr.off[p] + rows[p];
  }
  const int64_t n = pr.off[parts];
  if (n <= 0 || n >= (int64_t)INT32_MAX) return knn_fail(KNN_ERR_ARG, "total rows must be in [1, 2^31)");
  if (k <= 0 || k > n) return knn_fail(KNN_ERR_ARG, "k must be in [1, total rows]");
  if (nsel == 0) return KNN_OK;
  if (!d_D || !d_lab_all || !d_orow || !d_labels) return knn_fail(KNN_ERR_ARG, "null pointer");
  hipStream_t s = stream_of(ctx, stream);
  const int64_t per = tie_scratch_bytes(n, ctx->class_cnt);
  const int nwg = std::min<int>(tie_workgroups(ctx, per), nsel);
  if ((rc = ctx->tie_ws.ensure((size_t)(per * nwg)))) return rc;
  Sink sink{};
  sink.mode = MODE_SINGLE;
  sink.k = k;
  sink.labels = d_labels;
  sink.idx = d_idx;
  sink.dist = d_dist;
  sink.flags = d_flags;
  launch_tie_resolve(d_D, pr, nsel, d_lab_all, d_orow, ctx->class_cnt,
                     (unsigned char*)ctx->tie_ws.p, per, nwg, sink,
                     (unsigned long long*)ctx->totals.p + 2, s);
  HIP_TRY(hipGetLastError());
  return KNN_OK;
}

int knn_minmax_device(knn_ctx* ctx, const double* d_X, int64_t rows, int32_t d, double* d_max,
                      double* d_min, int32_t init, void* stream) {
  int rc;
  if ((rc = device_guard(ctx))) return rc;
  if (rows < 0 || d <= 0 || (rows > 0 && !d_X) || !d_max || !d_min)
    return knn_fail(KNN_ERR_ARG, "bad minmax arguments");
  hipStream_t s = stream_of(ctx, stream);
  const int64_t R = minmax_rows_per_sweep(rows, d, ctx->cu_count);
  if ((rc = ctx->nrm_part.ensure((size_t)2 * d * R * sizeof(double)))) return rc;
  launch_minmax(d_X, rows, d, R, (double*)ctx->nrm_part.p, d_max, d_min, init, s);
  HIP_TRY(hipGetLastError());
  return KNN_OK;
}

int knn_normalize_device(knn_ctx* ctx, double* d_X, int64_t rows, int32_t d,
                         const double* d_max, const double* d_min, void* stream) {
  int rc;
  if ((rc = device_guard(ctx))) return rc;
  if (rows < 0 || d <= 0 || (rows > 0 && !d_X) || !d_max || !d_min)
    return knn_fail(KNN_ERR_ARG, "bad normalize arguments");
  hipStream_t s = stream_of(ctx, stream);
  launch_normalize_apply(d_X, rows, d, minmax_rows_per_sweep(rows, d, ctx->cu_count), d_max,
                         d_min, s);
  HIP_TRY(hipGetLastError());
  return KNN_OK;
}

int knn_normalize(knn_ctx* ctx, double* const* sets, const int64_t* rows, int32_t nsets,
                  int32_t d, double* out_max, double* out_min) {
  int rc;
  if ((rc = device_guard(ctx))) return rc;
  if (nsets < 0 || d <= 0 || (nsets > 0 && (!sets || !rows)))
    return knn_fail(KNN_ERR_ARG, "bad normalize arguments");
  int64_t total = 0;
  for (int i = 0; i < nsets; i++) {
    if (rows[i] < 0 || (rows[i] > 0 && !sets[i])) return knn_fail(KNN_ERR_ARG, "bad set");
    total += rows[i];
  }
  hipStream_t s = ctx->stream;
  if ((rc = ctx->nrm_mm.ensure((size_t)2 * d * sizeof(double)))) return rc;
  if ((rc = ctx->nrm_X.ensure((size_t)std::max<int64_t>(total, 1) * d * sizeof(double)))) return rc;
  double* dmax = (double*)ctx->nrm_mm.p;
  double* dmin = dmax + d;
  double* dX = (double*)ctx->nrm_X.p;
  int64_t off = 0;
  for (int i = 0; i < nsets; i++) {  // cpp:245-274 over every set
    double* di = dX + off * d;
    if (rows[i] > 0)
      HIP_TRY(hipMemcpyAsync(di, sets[i], (size_t)rows[i] * d * sizeof(double),
                             hipMemcpyHostToDevice, s));
    if ((rc = knn_minmax_device(ctx, di, rows[i], d, dmax, dmin, i == 0, s))) return rc;
    off += rows[i];
  }
  if (nsets == 0 && (rc = knn_minmax_device(ctx, nullptr, 0, d, dmax, dmin, 1, s))) return rc;
  off = 0;
  for (int i = 0; i < nsets; i++) {  // cpp:279-305
    double* di = dX + off * d;
    if ((rc = knn_normalize_device(ctx, di, rows[i], d, dmax, dmin, s))) return rc;
    if (rows[i] > 0)
      HIP_TRY(hipMemcpyAsync(sets[i], di, (size_t)rows[i] * d * sizeof(double),
                             hipMemcpyDeviceToHost, s));
    off += rows[i];
  }
  if (out_max) HIP_TRY(hipMemcpyAsync(out_max, dmax, d * sizeof(double), hipMemcpyDeviceToHost, s));
  if (out_min) HIP_TRY(hipMemcpyAsync(out_min, dmin, d * sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return KNN_OK;
}

}  // extern "C"

// ---- CSV reader (knn_csv.hip, knn_csv_num.h; replaces cpp:154-222)

namespace {

using csv_clock = std::chrono::steady_clock;
double csv_secs(csv_clock::time_point a, csv_clock::time_point b) {
  return std::chrono::duration<double>(b - a).count();
}

// the conversion table, generated once per process and uploaded once per
// context (a blocking copy: complete for every stream when it returns)
int csv_ensure_table(knn_ctx* ctx) {
  if (ctx->csv_tab_ready) return KNN_OK;
  static const knncsv::NumTable* host = [] {
    auto* t = new knncsv::NumTable;
    knncsv::csv_build_num_table(t);
    return t;
  }();
  int rc;
  if ((rc = ctx->csv_tab.ensure(sizeof(knncsv::NumTable)))) return rc;
  HIP_TRY(hipMemcpy(ctx->csv_tab.p, host, sizeof(knncsv::NumTable), hipMemcpyHostToDevice));
  ctx->csv_tab_ready = true;
  return KNN_OK;
}

int csv_token_cap(int dim, bool with_label, int64_t rows, int64_t* cap) {
  const int64_t per = (int64_t)dim + (with_label ? 1 : 0);
  if (rows > INT64_MAX / per) return knn_fail(KNN_ERR_ARG, "rows * (dim [+ 1]) overflows");
  *cap = rows * per;
  return KNN_OK;
}

// count + scan + convert (convert alone when convert_only: the block bases of
// the previous call on the same text are still in the workspace); enqueue only
int csv_enqueue(knn_ctx* ctx, const char* d_text, int64_t bytes, int dim, bool with_label,
                int64_t cap, double* d_data, int32_t* d_labels, int64_t* d_tokens,
                int64_t* d_slow, int64_t slow_cap, int64_t* d_nslow, bool convert_only,
                hipStream_t s) {
  int rc;
  HIP_TRY(hipMemsetAsync(d_nslow, 0, sizeof(int64_t), s));
  if (bytes == 0) {
    HIP_TRY(hipMemsetAsync(d_tokens, 0, sizeof(int64_t), s));
    return KNN_OK;
  }
  if ((rc = csv_ensure_table(ctx))) return rc;
  const int64_t nblk = csv_block_count(bytes);
  if (nblk > (int64_t)INT32_MAX) return knn_fail(KNN_ERR_ARG, "CSV text too large");
  const size_t base_off = ((size_t)nblk * sizeof(unsigned int) + 15) & ~(size_t)15;
  if ((rc = ctx->csv_ws.ensure(base_off + (size_t)nblk * sizeof(int64_t)))) return rc;
  unsigned int* cnt = (unsigned int*)ctx->csv_ws.p;
  int64_t* base = (int64_t*)((char*)ctx->csv_ws.p + base_off);
  if (!convert_only) launch_csv_count_scan(d_text, bytes, cnt, base, d_tokens, s);
  launch_csv_convert(d_text, bytes, base, (const knncsv::NumTable*)ctx->csv_tab.p, dim, with_label,
                     cap, d_data, d_labels, d_slow, slow_cap, d_nslow, s);
  HIP_TRY(hipGetLastError());
  return KNN_OK;
}

// the whole file into buf (parallel pread of equal byte ranges, at most 16
// threads), 16 spare bytes behind it
int csv_slurp(const char* path, std::unique_ptr<char[]>& buf, int64_t* bytes) {
  const int fd = open(path, O_RDONLY);
  if (fd < 0) return knn_fail(KNN_ERR_ARG, std::string("cannot open ") + path);
  struct stat st;
  if (fstat(fd, &st) != 0 || st.st_size < 0 || !S_ISREG(st.st_mode)) {
    close(fd);
    return knn_fail(KNN_ERR_ARG, std::string("cannot size ") + path);
  }
  const size_t sz = (size_t)st.st_size;
  buf.reset(new char[sz + 16]);
  int threads = (int)std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
  if (sz < (1u << 20)) threads = 1;
  std::vector<int> bad(threads, 0);
  const auto part = [&](int t) {
    size_t o = sz * t / threads;
    const size_t end = sz * (t + 1) / threads;
    while (o < end) {
      const ssize_t got = pread(fd, buf.get() + o, end - o, (off_t)o);
      if (got <= 0) {
        bad[t] = 1;
        return;
      }
      o += (size_t)got;
    }
  };
  {
    std::vector<std::thread> th;
    for (int t = 1; t < threads; t++) th.emplace_back(part, t);
    part(0);
    for (auto& x : th) x.join();
  }
  close(fd);
  for (int t = 0; t < threads; t++)
    if (bad[t]) return knn_fail(KNN_ERR_ARG, std::string("short read on ") + path);
  *bytes = (int64_t)sz;
  return KNN_OK;
}

// File -> device values: reads and uploads the text, parses it into d_data /
// d_labels and fetches the slow list (every slow token: the convert step runs
// once more when the first capacity was too small).  Waits for the device.
int csv_read_core(knn_ctx* ctx, const char* path, int dim, bool with_label, int64_t rows,
                  int64_t cap, double* d_data, int32_t* d_labels, std::unique_ptr<char[]>& buf,
                  int64_t* bytes, std::vector<int64_t>& slow, int64_t* tokens) {
  int rc;
  hipStream_t s = ctx->stream;
  for (double& v : ctx->csv_phase_s) v = 0.0;
  ctx->csv_last_slow = -1;
  const auto t0 = csv_clock::now();
  if ((rc = csv_slurp(path, buf, bytes))) return rc;
  const auto t1 = csv_clock::now();
  if ((rc = ctx->csv_text.ensure((size_t)*bytes + 16))) return rc;
  if (*bytes > 0)
    HIP_TRY(hipMemcpyAsync(ctx->csv_text.p, buf.get(), (size_t)*bytes, hipMemcpyHostToDevice, s));
  HIP_TRY(hipStreamSynchronize(s));
  const auto t2 = csv_clock::now();
  int64_t slow_cap = std::max<int64_t>(4096, *bytes / 64);
  if ((rc = ctx->csv_slow.ensure((size_t)slow_cap * 2 * sizeof(int64_t)))) return rc;
  if ((rc = ctx->csv_misc.ensure(2 * sizeof(int64_t)))) return rc;
  int64_t* misc = (int64_t*)ctx->csv_misc.p;  // {tokens, slow count}
  int64_t h[2] = {0, 0};
  for (int pass = 0; pass < 2; ++pass) {
    if ((rc = csv_enqueue(ctx, (const char*)ctx->csv_text.p, *bytes, dim, with_label, cap, d_data,
                          d_labels, misc, (int64_t*)ctx->csv_slow.p, slow_cap, misc + 1, pass == 1,
                          s)))
      return rc;
    HIP_TRY(hipMemcpyAsync(h, misc, sizeof h, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (h[1] <= slow_cap) break;
    if (pass == 1) return knn_fail(KNN_ERR_DEVICE, "CSV slow list overflowed twice");
    slow_cap = h[1];  // every slow token this time
    if ((rc = ctx->csv_slow.ensure((size_t)slow_cap * 2 * sizeof(int64_t)))) return rc;
  }
  slow.resize((size_t)h[1] * 2);
  if (h[1] > 0) {
    HIP_TRY(hipMemcpyAsync(slow.data(), ctx->csv_slow.p, slow.size() * sizeof(int64_t),
                           hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
  }
  const auto t3 = csv_clock::now();
  *tokens = h[0];
  ctx->csv_last_slow = h[1];
  ctx->csv_phase_s[0] = csv_secs(t0, t1);
  ctx->csv_phase_s[1] = csv_secs(t1, t2);
  ctx->csv_phase_s[2] = csv_secs(t2, t3);
  return KNN_OK;
}

// atof / atoi of slow token (c, p), as the reference runs them: on a
// NUL-terminated copy of the token, whose start is found backwards from its
// terminator p.  Returns the fp64 bits or the int32 value.
int64_t csv_slow_value(const char* text, int64_t p, bool is_label, std::string& tok) {
  int64_t b = p;
  while (b > 0 && text[b - 1] != ',' && text[b - 1] != '\n') --b;
  tok.assign(text + b, text + p);
  if (is_label) return (int64_t)atoi(tok.c_str());
  const double v = atof(tok.c_str());
  int64_t bits;
  memcpy(&bits, &v, sizeof bits);
  return bits;
}

int csv_check_read_args(const char* path, int dim, int64_t rows, const void* data,
                        bool with_label, const void* labels, const int64_t* tokens) {
  if (!path) return knn_fail(KNN_ERR_ARG, "null path");
  if (dim < 1) return knn_fail(KNN_ERR_ARG, "dim must be >= 1");
  if (rows < 0) return knn_fail(KNN_ERR_ARG, "rows must be >= 0");
  if (rows > 0 && !data) return knn_fail(KNN_ERR_ARG, "null data");
  if (with_label && rows > 0 && !labels) return knn_fail(KNN_ERR_ARG, "null labels (with_label)");
  if (!tokens) return knn_fail(KNN_ERR_ARG, "null tokens");
  return KNN_OK;
}

}  // namespace

extern "C" {

int knn_csv_parse_device(knn_ctx* ctx, const char* d_text, int64_t bytes, int32_t dim,
                         int32_t with_label, int64_t rows, double* d_data, int32_t* d_labels,
                         int64_t* d_tokens, int64_t* d_slow, int64_t slow_cap, int64_t* d_nslow,
                         void* stream) {
  int rc;
  if ((rc = device_guard(ctx))) return rc;
  if (dim < 1) return knn_fail(KNN_ERR_ARG, "dim must be >= 1");
  if (rows < 0) return knn_fail(KNN_ERR_ARG, "rows must be >= 0");
  if (bytes < 0) return knn_fail(KNN_ERR_ARG, "bytes must be >= 0");
  if (bytes > 0 && !d_text) return knn_fail(KNN_ERR_ARG, "null d_text");
  if ((uintptr_t)d_text & 15) return knn_fail(KNN_ERR_ARG, "d_text must be 16-byte aligned");
  if (rows > 0 && !d_data) return knn_fail(KNN_ERR_ARG, "null d_data");
  if (with_label && rows > 0 && !d_labels)
    return knn_fail(KNN_ERR_ARG, "null d_labels (with_label)");
  if (!d_tokens || !d_nslow) return knn_fail(KNN_ERR_ARG, "null d_tokens / d_nslow");
  if (slow_cap < 0 || (slow_cap > 0 && !d_slow))
    return knn_fail(KNN_ERR_ARG, "bad slow list (slow_cap < 0, or null d_slow)");
  int64_t cap;
  if ((rc = csv_token_cap(dim, with_label != 0, rows, &cap))) return rc;
  hipStream_t s = stream_of(ctx, stream);
  return csv_enqueue(ctx, d_text, bytes, dim, with_label != 0, cap, d_data, d_labels, d_tokens,
                     d_slow, slow_cap, d_nslow, false, s);
}

int knn_csv_read(knn_ctx* ctx, const char* path, int32_t dim, int32_t with_label, int64_t rows,
                 double* data, int32_t* labels, int64_t* tokens) {
  int rc;
  if ((rc = device_guard(ctx))) return rc;
  if ((rc = csv_check_read_args(path, dim, rows, data, with_label != 0, labels, tokens))) return rc;
  const bool wl = with_label != 0;
  int64_t cap;
  if ((rc = csv_token_cap(dim, wl, rows, &cap))) return rc;
  if ((rc = ctx->csv_data.ensure((size_t)rows * dim * sizeof(double)))) return rc;
  if ((rc = ctx->csv_lab.ensure((size_t)rows * sizeof(int32_t)))) return rc;
  std::unique_ptr<char[]> buf;
  std::vector<int64_t> slow;
  int64_t bytes = 0;
  if ((rc = csv_read_core(ctx, path, dim, wl, rows, cap, (double*)ctx->csv_data.p,
                          (int32_t*)ctx->csv_lab.p, buf, &bytes, slow, tokens)))
    return rc;
  // the cells tokens reached are a prefix of each array; the rest stays as it was
  const auto t3 = csv_clock::now();
  hipStream_t s = ctx->stream;
  const int64_t stored = std::min(*tokens, cap);
  const int64_t nlab = wl ? (stored + dim) / ((int64_t)dim + 1) : 0;
  const int64_t ndata = stored - nlab;
  if (ndata > 0)
    HIP_TRY(hipMemcpyAsync(data, ctx->csv_data.p, (size_t)ndata * sizeof(double),
                           hipMemcpyDeviceToHost, s));
  if (nlab > 0)
    HIP_TRY(hipMemcpyAsync(labels, ctx->csv_lab.p, (size_t)nlab * sizeof(int32_t),
                           hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  const auto t4 = csv_clock::now();
  std::string tok;
  for (size_t i = 0; i + 1 < slow.size(); i += 2) {
    const int64_t c = slow[i], p = slow[i + 1];
    if (c < 0 || c >= cap || p < 0 || p > bytes) continue;
    const int64_t row = wl ? c / ((int64_t)dim + 1) : 0;
    const bool is_label = wl && c - row * ((int64_t)dim + 1) == 0;
    const int64_t v = csv_slow_value(buf.get(), p, is_label, tok);
    if (is_label)
      labels[row] = (int32_t)v;
    else
      memcpy(&data[wl ? c - row - 1 : c], &v, sizeof v);
  }
  ctx->csv_phase_s[3] = csv_secs(t3, t4);
  ctx->csv_phase_s[4] = csv_secs(t4, csv_clock::now());
  return KNN_OK;
}

int knn_csv_read_device(knn_ctx* ctx, const char* path, int32_t dim, int32_t with_label,
                        int64_t rows, double* d_data, int32_t* d_labels, int64_t* tokens) {
  int rc;
  if ((rc = device_guard(ctx))) return rc;
  if ((rc = csv_check_read_args(path, dim, rows, d_data, with_label != 0, d_labels, tokens)))
    return rc;
  const bool wl = with_label != 0;
  int64_t cap;
  if ((rc = csv_token_cap(dim, wl, rows, &cap))) return rc;
  std::unique_ptr<char[]> buf;
  std::vector<int64_t> slow;
  int64_t bytes = 0;
  if ((rc = csv_read_core(ctx, path, dim, wl, rows, cap, d_data, d_labels, buf, &bytes, slow,
                          tokens)))
    return rc;
  const auto t4 = csv_clock::now();
  std::string tok;
  for (size_t i = 0; i + 1 < slow.size(); i += 2) {  // (c, p) -> (c, value)
    const int64_t c = slow[i], p = slow[i + 1];
    if (c < 0 || c >= cap || p < 0 || p > bytes) {
      slow[i] = -1;
      continue;
    }
    const bool is_label = wl && c % ((int64_t)dim + 1) == 0;
    slow[i + 1] = csv_slow_value(buf.get(), p, is_label, tok);
  }
  if (!slow.empty()) {
    hipStream_t s = ctx->stream;
    if ((rc = ctx->csv_fix.ensure(slow.size() * sizeof(int64_t)))) return rc;
    HIP_TRY(hipMemcpyAsync(ctx->csv_fix.p, slow.data(), slow.size() * sizeof(int64_t),
                           hipMemcpyHostToDevice, s));
    launch_csv_scatter((const int64_t*)ctx->csv_fix.p, (int64_t)(slow.size() / 2), dim, wl, cap,
                       d_data, d_labels, s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));
  }
  ctx->csv_phase_s[4] = csv_secs(t4, csv_clock::now());
  return KNN_OK;
}

int64_t knn_csv_last_slow(knn_ctx* ctx) { return ctx ? ctx->csv_last_slow : -1; }

int knn_csv_last_phases(knn_ctx* ctx, double out_s[5]) {
  if (!ctx || !out_s) return knn_fail(KNN_ERR_ARG, "null context / output");
  for (int i = 0; i < 5; i++) out_s[i] = ctx->csv_phase_s[i];
  return KNN_OK;
}

int knn_sync(knn_ctx* ctx) {
  int rc;
  if ((rc = device_guard(ctx))) return rc;
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  HIP_TRY(hipEventSynchronize(ctx->done_ev));  // the last call, on whatever stream it ran
  auto_check(ctx);
  return KNN_OK;
}

int64_t knn_last_rescan_count(knn_ctx* ctx) {
  if (!ctx || hipSetDevice(ctx->device) != hipSuccess) return -1;
  if (hipEventSynchronize(ctx->done_ev) != hipSuccess) return -1;  // the last call's counts
  auto_check(ctx);
  return ctx->h_counts[0];
}

int knn_rescan_totals(knn_ctx* ctx, int64_t out[2], int reset) {
  int rc;
  if ((rc = device_guard(ctx))) return rc;
  if (!out) return knn_fail(KNN_ERR_ARG, "null output");
  unsigned long long v[2];
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  HIP_TRY(hipEventSynchronize(ctx->done_ev));
  HIP_TRY(hipMemcpy(v, ctx->totals.p, sizeof v, hipMemcpyDeviceToHost));
  out[0] = (int64_t)v[0];
  out[1] = (int64_t)v[1];
  if (reset) HIP_TRY(hipMemset(ctx->totals.p, 0, sizeof v));
  auto_check(ctx);
  return KNN_OK;
}

int knn_tie_totals(knn_ctx* ctx, int64_t* out, int reset) {
  int rc;
  if ((rc = device_guard(ctx))) return rc;
  if (!out) return knn_fail(KNN_ERR_ARG, "null output");
  unsigned long long v = 0;
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  HIP_TRY(hipEventSynchronize(ctx->done_ev));
  HIP_TRY(hipMemcpy(&v, (unsigned long long*)ctx->totals.p + 2, sizeof v, hipMemcpyDeviceToHost));
  *out = (int64_t)v;
  if (reset) HIP_TRY(hipMemset((unsigned long long*)ctx->totals.p + 2, 0, sizeof v));
  return KNN_OK;
}

const char* knn_last_kernel_name(knn_ctx* ctx) { return ctx ? ctx->last_kernel : ""; }

int knn_set_precision(knn_ctx* ctx, int mode) {
  if (!ctx) return knn_fail(KNN_ERR_ARG, "null context");
  if (mode < KNN_PRECISION_AUTO || mode > KNN_PRECISION_FP16)
    return knn_fail(KNN_ERR_ARG, "unknown precision mode");
  ctx->precision = mode;
  return KNN_OK;
}

int knn_set_vote(knn_ctx* ctx, int mode) {
  if (!ctx) return knn_fail(KNN_ERR_ARG, "null context");
  if (mode != KNN_VOTE_UNIFORM && mode != KNN_VOTE_DISTANCE)
    return knn_fail(KNN_ERR_ARG, "unknown vote mode " + std::to_string(mode) +
                                     " (0 uniform, 1 distance)");
  ctx->vote = mode;
  return KNN_OK;
}

int knn_get_vote(knn_ctx* ctx) { return ctx ? ctx->vote : -1; }

int knn_last_candidate_path(knn_ctx* ctx) { return ctx ? ctx->last_kmetric : -1; }

int knn_set_tuning(knn_ctx* ctx, const char* key, int64_t value) {
  if (!ctx || !key) return knn_fail(KNN_ERR_ARG, "null argument");
  const char* err;
  const int rc = set_tuning(ctx->tune, key, value, &err);
  if (rc) return knn_fail(rc, err ? err : std::string("unknown tuning key ") + key);
  return KNN_OK;
}

int knn_set_timing(knn_ctx* ctx, int enable) {
  int rc;
  if ((rc = device_guard(ctx))) return rc;
  // timing-only events: no system-scope fence (cache writeback and
  // invalidate) at each record -- with it every record idled the stream
  // ~6 us (profiles/ab_log.md r5u); only the times are read back
  if (enable < 0 || enable > 2) return knn_fail(KNN_ERR_ARG, "timing must be 0, 1 or 2");
  if (enable && !ctx->ring[0].ev[0])
    for (auto& tc : ctx->ring)
      for (auto& e : tc.ev) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableSystemFence));
  ctx->timing = enable;
  return KNN_OK;
}

double knn_last_phase_ms(knn_ctx* ctx, int phase) {
  if (!ctx || phase < 0 || phase > 3 || ctx->ring_last < 0) return -1.0;
  if (hipSetDevice(ctx->device) != hipSuccess) return -1.0;
  TimedCall& tc = ctx->ring[ctx->ring_last];
  if (!phase_timed(tc, phase)) return -1.0;
  if (hipEventSynchronize(tc.ev[tc.mode == 2 ? 2 : 4]) != hipSuccess) return -1.0;
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, tc.ev[phase], tc.ev[phase + 1]) != hipSuccess) return -1.0;
  return ms;
}

int knn_timing_totals(knn_ctx* ctx, double out_ms[4], int64_t* calls, int reset) {
  int rc;
  if ((rc = device_guard(ctx))) return rc;
  for (auto& tc : ctx->ring) fold_timing(ctx, tc);
  if (out_ms)
    for (int p = 0; p < 4; p++) out_ms[p] = ctx->tsum[p];
  if (calls) *calls = ctx->tcalls;
  if (reset) {
    for (double& v : ctx->tsum) v = 0.0;
    ctx->tcalls = 0;
  }
  return KNN_OK;
}

int knn_last_geometry(knn_ctx* ctx, int64_t out[4]) {
  if (!ctx || !out) return knn_fail(KNN_ERR_ARG, "null argument");
  for (int i = 0; i < 4; i++) out[i] = ctx->geom[i];
  return KNN_OK;
}

}  // extern "C"
