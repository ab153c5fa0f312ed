// knn_dims.h -- the dimensions and padding rules that the kernels and the
// host-only search plan (knn_plan.h) share.  Plain C++: no HIP types, so the
// plan and its checker compile without a device toolchain.
#pragma once
#include <stdint.h>

namespace knnk {

constexpr int kQPB = 128;        // queries per candidate workgroup (4 waves x 32)
constexpr int kMaxUnion = 1024;  // max candidates kept per query across all lists
constexpr int kStreamDC = 32;    // dims per LDS chunk in the large-d kernel
constexpr int kS3Rows = 256;        // S3 kernel: train rows per tile = queries per workgroup
constexpr int kS3GqMax = 4;         // S3: default largest XCD grouping of query tiles (s3_group)
constexpr int kGthrSlots = 8;                // slots per query in gthr
constexpr int kRescanFastQueries = 65536;  // failed queries per call the fast path serves
constexpr int kRegionMax = 64;  // regions (k-means centroids) at most
constexpr int kNormWin = 16384;

int pad_dim(int d);                 // padded dim the candidate kernels run at
int pad_dim_bf16x3(int d);          // padded dim of the bf16x3 kernel, -1 if unsupported
int pad_dim_fp16(int d);            // padded dim of the fp16 kernel (metric 4), -1 if unsupported
bool bf16x3_streamed(int DP);       // bf16x3 at this DP runs the S3 stream kernel
// S3 workgroup grouping for n_qt query tiles and S splits (knn_cand.hip, s3_map)
int s3_group(int n_qt, int S, int gq_max = kS3GqMax);
int pad_dim_fp16_s3(int d);         // padded dim of the fp16 S3 image (multiple of 32, > 256)
bool cand_supported(int DP);
int pad_dim_i8(int d);  // padded dim of the int8 kernel (a multiple of 64, <= 256), -1 if none
int pad_dim_i8w(int d); // padded dim of the int8 32x32x32 kernel (metric 6), -1 if none
// padded dim of the wide L1-on-codes image (knn_cand_sad_wide.hip): d in (256, 1024]
// rounded up to the kernel's 16-dim granule, -1 outside
int pad_dim_i8l1w(int d);
// padded dim of the 16-bit fixed-point L1 image (knn_cand_fix16.hip): a
// multiple of 32 up to 256 (65535 * 256 < 2^24: the sums stay exact floats),
// -1 beyond
int pad_dim_u16l1(int d);
// padded dim of the wide 16-bit fixed-point L1 image (knn_cand_fix16_wide.hip):
// d in (256, 1024] rounded up to 16, -1 outside.  65535 * 1024 < 2^26: the
// sums are exact integers and floats within fix16_wide_round code units
int pad_dim_u16l1w(int d);
// |fl32(P) - P| at most, for a sum P of DP code differences (code units): 0
// below 2^24 (DP <= 256), half an ulp of [2^24, 2^25) up to DP = 512, of
// [2^25, 2^26) up to DP = 1024
constexpr int fix16_wide_round(int DP) { return DP <= 256 ? 0 : DP <= 512 ? 1 : 2; }
// that image's dim slabs: a row of cpr 16-byte chunks (8 codes each) is one
// slab up to 64 chunks (512 dims), two halves above; chunks of the first slab
constexpr int fix16_wide_slab0(int cpr) { return cpr > 64 ? (cpr + 1) / 2 : cpr; }

// Queries per pass of the fast rescan's filter above 256 dims
// (rescan_filter_wide_kernel, knn_select.hip) at padded width DP: the largest
// of 8, 4, 2, 1 whose rows and thresholds, FQW (DP + 1) floats, fit lds_limit
// bytes beside the kernel's own variables (8 FQW + 8 bytes; 128 reserved); 0
// where not even one query fits (no filter then: the full scan takes every
// failed query)
int rescan_wide_queries(int DP, int64_t lds_limit);

#define KNN_DP_LIST(X) X(8) X(16) X(24) X(32) X(48) X(64) X(96) X(128) X(160) X(192) X(256)

}  // namespace knnk
