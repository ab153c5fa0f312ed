/* knn_amd.h -- C ABI of the MI355X-native brute-force KNN classifier.
 *
 * This is the drop-in boundary for the hot path of Jason-Woo/-MPI-KNN-
 * (/root/reference/knn_mpi.cpp, cited "cpp:N").  The reference has no
 * library interface: its hot path is inlined in main() (cpp:308-381), fed by
 * the constant block (cpp:108-119) and the MPI collectives (cpp:224-227,
 * 340, 383).  Each entry point below replaces one piece of that:
 *
 *   knn_set_train*      MPI_Bcast of Data_train/Train_label (cpp:224-225) and
 *                       the train side of the config block (N_train, dim,
 *                       class_cnt: cpp:108-113)
 *   knn_classify*       the query loop: per-pair Euclidean_D/Manhattan_D
 *                       (cpp:33-67) -> std::sort of all N_train records
 *                       (cpp:323/366) -> first-to-max vote over K
 *                       (cpp:324-337/367-380) -> Val/Test_label_buffer
 *   knn_search_partial  train-sharded variant (new; north_star mode b):
 *                       exact local top-w per query with global indices
 *   knn_merge_vote      k-way merge of per-shard lists + the vote (cpp:324-337)
 *   knn_group_*         single-process multi-GPU driver over RCCL/xGMI that
 *                       replaces MPI_Bcast/Scatter/Gather (cpp:224-227, 383)
 *
 * Semantics (identical to the reference on the same fp64 inputs):
 *   - distances are the reference's fp64 values: sqrt of the sequential
 *     sum of (q_i - x_i)^2 (no FMA) for metric 0, sum of |q_i - x_i| for
 *     metric 1;
 *   - neighbours are ordered by ascending distance.  Among exactly equal
 *     distances the reference's order is whatever its std::sort (libstdc++
 *     introsort) leaves; queries where that order can change the label
 *     (KNN_FLAG_TIE_VOTE / KNN_FLAG_TIE_BOUNDARY) are re-ordered exactly as
 *     the reference's std::sort orders them (KNN_FLAG_TIE_REF), other ties
 *     are ordered by train index (KNN_FLAG_TIE_ORDER; tuning key "ties" = 2
 *     re-orders those too);
 *   - label = first label whose running count strictly exceeds the running
 *     maximum while scanning the k nearest in order; -1 when k == 0.
 *   - the GPU computes a certified candidate set on MFMA (by default exact
 *     int8 codes on v_mfma_i32_16x16x64_i8 / 32x32x32_i8 for integer-coded
 *     train sets,
 *     else fp16 operands on v_mfma_f32_16x16x32_f16; bf16x3 or fp32 by
 *     precision mode, see knn_set_precision) and re-ranks it in fp64; queries whose
 *     candidate set cannot be certified are re-run exactly (fp64 over all
 *     rows).  No CPU fallback exists: without a usable HIP device every call
 *     fails with KNN_ERR_DEVICE.
 *
 * Conventions: plain pointers and sizes; return 0 on success, a negative
 * KNN_ERR_* code on failure (message via knn_last_error(), thread-local).
 * A host driver maps non-zero to exit(1), like MPI_Abort(..., 1)
 * (cpp:127-129).  One host thread per context; contexts are independent.
 * "Host" pointers are ordinary CPU memory; "_device" variants take device
 * pointers on the context's GPU and an optional hipStream_t (NULL = the
 * context's own stream, which is ordered after work on the device's legacy
 * default stream; work on other streams must be synchronised by the caller).
 */
#ifndef KNN_AMD_H
#define KNN_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KNN_OK 0
#define KNN_ERR_ARG -1     /* bad argument (sizes, k > n_train, label range) */
#define KNN_ERR_DEVICE -2  /* no HIP device / HIP runtime error */
#define KNN_ERR_STATE -3   /* e.g. classify before set_train */
#define KNN_ERR_NOMEM -4   /* device allocation failed */
#define KNN_ERR_COMM -5    /* RCCL failure */

/* bytes of CSV text one workgroup of the reader owns (knn_csv_parse_device) */
#define KNN_CSV_BLOCK_BYTES 16384

#define KNN_METRIC_L2 0 /* Euclidean_distance = true  (cpp:114, 320, 363) */
#define KNN_METRIC_L1 1 /* Euclidean_distance = false (cpp:114, 321, 364) */

/* out_flags bits (per query) */
#define KNN_FLAG_EXACT_RESCAN 1 /* candidate set not certified; exact fp64 rescan used */
#define KNN_FLAG_TIE_BOUNDARY 2 /* dist[k-1] == dist[k]: membership tie at the k-th */
#define KNN_FLAG_TIE_VOTE 4     /* equal distances with different labels inside top-k */
#define KNN_FLAG_TIE_ORDER 8    /* equal distances inside top-k (order unspecified in
                                   the reference's std::sort; ours: by train index) */
#define KNN_FLAG_NONFINITE 16   /* the query has a NaN / inf coordinate: label -1, no
                                   neighbours (idx -1, dist NaN); the reference's
                                   distances are undefined there */
#define KNN_FLAG_TIE_REF 32     /* a tied query re-ordered as the reference's std::sort
                                   orders it (libstdc++ introsort emulated over all
                                   n distances): label, indices and their order are
                                   the reference's (knn_set_tuning "ties") */
#define KNN_FLAG_TIE_PENDING 64 /* knn_merge_vote_device: the label can depend on the
                                   reference's order among equal distances ACROSS
                                   shards; knn_shard_distances_device +
                                   knn_tie_resolve_device give the reference's order
                                   (knn_group mode 1 does this itself) */

typedef struct knn_ctx knn_ctx;
typedef struct knn_group knn_group;

/* Version string of the library build. */
const char* knn_version(void);
/* Last error message of the calling thread ("" if none). */
const char* knn_last_error(void);
/* Number of visible HIP devices (0 if none). */
int knn_device_count(void);

/* Context on HIP device `device` (replaces MPI_Init + per-rank state, cpp:123-125). */
int knn_create(knn_ctx** out, int device);
int knn_destroy(knn_ctx* ctx);

/* Train set from host memory: X row-major n x d fp64 (Data_train, cpp:140),
 * labels (Train_label, cpp:141) with 0 <= label < class_cnt.  The library
 * copies both to HBM (≙ MPI_Bcast cpp:224-225).  KNN_ERR_ARG for a label out
 * of range or a non-finite value (NaN / inf) anywhere in X, and for a train
 * set with |x - mean| >= 2^400 in any dimension (mean: the dimension's mean
 * over the train rows; beyond that the candidate passes' operands could
 * overflow).  A refused train set leaves the context without one: classify
 * returns KNN_ERR_STATE until a set_train succeeds. */
int knn_set_train(knn_ctx* ctx, const double* X, const int32_t* labels, int64_t n,
                  int32_t d, int32_t class_cnt);
/* Same from device memory on ctx's GPU (e.g. after an RCCL broadcast).
 * dX/dlabels are borrowed and must stay valid until the next set_train or
 * destroy.  idx_offset is added to every reported neighbour index (train
 * sharding: global index of this shard's first row).  Labels and values are
 * checked on the device (same errors as knn_set_train).  The work runs on
 * the context's stream, which is ordered after the device's legacy default
 * stream: producers on other streams must be synchronised by the caller. */
int knn_set_train_device(knn_ctx* ctx, const double* dX, const int32_t* dlabels, int64_t n,
                         int32_t d, int32_t class_cnt, int64_t idx_offset);

/* Classify m queries Q (row-major m x d fp64, same d as the train set).
 * out_labels[m] (Test_label_buffer, cpp:380) required; out_idx[m*k]
 * (global train indices) and out_dist[m*k] (fp64 reference distances) and
 * out_flags[m] nullable.  Host pointers.  0 <= k <= n_train (k > 1000 runs
 * the exact large-k path). */
int knn_classify(knn_ctx* ctx, const double* Q, int64_t m, int32_t k, int32_t metric,
                 int32_t* out_labels, int64_t* out_idx, double* out_dist,
                 int32_t* out_flags);
/* Device-pointer variant; enqueued on `stream` (hipStream_t, NULL = ctx
 * stream) and returns without waiting for the device on every path: the
 * exact rescan of uncertified queries is enqueued too and sized on the
 * device.  Outputs are complete once the stream reaches the end of the call
 * (knn_sync, or any later work on the same stream).  One stream at a time
 * per context (the context's workspace is shared by its calls). */
int knn_classify_device(knn_ctx* ctx, const double* dQ, int64_t m, int32_t k, int32_t metric,
                        int32_t* d_labels, int64_t* d_idx, double* d_dist, int32_t* d_flags,
                        void* stream);

/* ---- K sweep: labels (and accuracy counts) for a list of K from ONE search.
 * The reference judges K by its validation pass (cpp:308-343), one run per
 * compiled-in K.  Its neighbour order does not depend on K (std::sort over
 * all N_train records, cpp:323; the vote scans the first K, cpp:324-337), so
 * the label at every K <= kmax is a prefix vote over one ordered top-kmax
 * row: these calls search once at kmax = max(ks) and vote every prefix.
 * ks: host array of nk values in any order, duplicates allowed, 1 <= nk <=
 * 4096, 0 <= ks[i] <= n_train (KNN_ERR_ARG names the offending entry).
 * Labels are laid out [nk][m]: row i belongs to ks[i] and equals what
 * knn_classify returns for k = ks[i] (K = 0: -1; a non-finite query: -1 at
 * every K).  truth [m] (nullable) are the queries' true labels: correct[i]
 * (int64, [nk]) then receives #{q : labels[i][q] == truth[q]} (≙ cnt of
 * cpp:341-343 per K); truth and correct go together (KNN_ERR_ARG otherwise).
 * Ties: with "ties" = 1 the queries whose label AT ANY K of the list the
 * reference's order among equal distances could change are re-ordered as its
 * std::sort orders them (KNN_FLAG_TIE_REF; "ties" = 2: every query with equal
 * distances in its top kmax; 0: none).
 *
 * knn_vote_sweep_device: the prefix votes alone, over caller-supplied ordered
 * neighbour rows d_idx [m][kmax] (global indices; -1 = empty slot, a row
 * starting with -1 gets -1 at every K) with label d_lab[idx - idx_base]
 * (building block; also for callers that merged lists themselves).  Here
 * ks[i] <= kmax.  Device pointers except ks; enqueue only. */
int knn_vote_sweep_device(knn_ctx* ctx, const int64_t* d_idx, int64_t m, int32_t kmax,
                          const int32_t* d_lab, int64_t idx_base, const int32_t* ks, int32_t nk,
                          int32_t* d_labels, const int32_t* d_truth, int64_t* d_correct,
                          void* stream);
/* Search at kmax = max(ks), sweep tie scan, reference-order pass, prefix
 * votes: enqueued on `stream` like knn_classify_device (no host wait).
 * d_labels [nk*m] required; d_truth / d_correct as above; d_idx / d_dist
 * [m*kmax] and d_flags [m] nullable (internal rows are used when null): the
 * top kmax of each query and the tie bits for kmax, KNN_FLAG_TIE_REF on the
 * rows the sweep re-ordered.  KNN_ERR_STATE before set_train. */
int knn_classify_sweep_device(knn_ctx* ctx, const double* dQ, int64_t m, const int32_t* ks,
                              int32_t nk, int32_t metric, int32_t* d_labels,
                              const int32_t* d_truth, int64_t* d_correct, int64_t* d_idx,
                              double* d_dist, int32_t* d_flags, void* stream);
/* Host-pointer twin (waits for the result): out_labels [nk*m], out_correct
 * [nk] (required iff truth), out_idx / out_dist [m*kmax], out_flags [m]
 * nullable. */
int knn_classify_sweep(knn_ctx* ctx, const double* Q, int64_t m, const int32_t* ks, int32_t nk,
                       int32_t metric, int32_t* out_labels, const int32_t* truth,
                       int64_t* out_correct, int64_t* out_idx, double* out_dist,
                       int32_t* out_flags);

/* ---- K sweep under exclusion / leave-one-out: score every K on the train
 * set itself.  The reference judges K on a separate validation CSV
 * (Validation, cpp:308-343); classifying the train rows against themselves
 * instead finds every row at distance 0 (K = 1 scores 100 %).  These calls
 * take one train row out of a query's neighbour search.  One rule fixes every
 * output: for a query with excluded global train index e the result is what
 * knn_classify_sweep returns on a context whose train set is the current one
 * WITH ROW e REMOVED (labels lose the same entry), reported indices >= e
 * shifted back up by one so every index refers to the full train set.  That
 * covers the label at every K, the neighbour indices, their order and the
 * distances, the flag bits KNN_FLAG_TIE_BOUNDARY | TIE_VOTE | TIE_ORDER |
 * TIE_REF and the rows "ties" = 0 / 1 / 2 re-order: the order among equal
 * distances is the reference's std::sort over the n - 1 remaining records
 * (cpp:323), another introsort run than the one over all n.
 * KNN_FLAG_EXACT_RESCAN may differ (certification is not part of the
 * contract).  One search at max(ks) + 1 serves the call.
 *
 * knn_classify_sweep_excl_device: knn_classify_sweep_device plus d_excl [m]
 * (device, global indices as reported in d_idx, i.e. with the train set's
 * idx_offset; -1 = exclude nothing: that query equals the plain sweep's).  A
 * value outside {-1} and [idx_offset, idx_offset + n_train) is treated as -1.
 * d_excl NULL = none for all queries (the plain sweep).  With d_excl non-NULL
 * ks[i] <= n_train - 1 (KNN_ERR_ARG names the offending entry).  Enqueue only. */
int knn_classify_sweep_excl_device(knn_ctx* ctx, const double* dQ, int64_t m,
                                   const int64_t* d_excl, const int32_t* ks, int32_t nk,
                                   int32_t metric, int32_t* d_labels, const int32_t* d_truth,
                                   int64_t* d_correct, int64_t* d_idx, double* d_dist,
                                   int32_t* d_flags, void* stream);
/* Leave-one-out over train rows [row0, row0 + rows) of the context (local row
 * numbers; KNN_ERR_ARG for a range outside [0, n_train]): the queries are the
 * context's own fp64 train rows, query i excludes global index idx_offset +
 * row0 + i and its truth is the label of row row0 + i (≙ Val_label against
 * Val_label_buffer, cpp:341-343).  d_labels [nk*rows] required; d_correct
 * [nk] nullable; d_idx / d_dist [rows*kmax], d_flags [rows] nullable.
 * 0 <= ks[i] <= n_train - 1.  Enqueue only. */
int knn_loo_sweep_device(knn_ctx* ctx, int64_t row0, int64_t rows, const int32_t* ks, int32_t nk,
                         int32_t metric, int32_t* d_labels, int64_t* d_correct, int64_t* d_idx,
                         double* d_dist, int32_t* d_flags, void* stream);
/* Host twin over all n_train rows (waits for the result): out_labels [nk][n]
 * required, out_correct [nk] (the leave-one-out cnt of cpp:341-343 per K),
 * out_idx / out_dist [n*kmax], out_flags [n] nullable.  Runs
 * knn_loo_sweep_device over fixed batches of at most 16384 rows, so the
 * workspace does not grow with n; out_correct is summed over the batches. */
int knn_loo_sweep(knn_ctx* ctx, const int32_t* ks, int32_t nk, int32_t metric, int32_t* out_labels,
                  int64_t* out_correct, int64_t* out_idx, double* out_dist, int32_t* out_flags);

/* ---- per-class evaluation: the confusion matrix at every K, vote counts.
 * The reference reports one cnt per run (cpp:341-343).  These calls report,
 * for every K of a sweep, the C x C confusion matrix
 *   conf[i][t][p] = #{q : truth[q] == t and labels[i][q] == p}   (int64,
 *   [nk][C][C], row = true class, column = predicted class),
 *   unl[i] = #{q : labels[i][q] or truth[q] outside [0, C)}       (int64, [nk])
 * (label -1 at K = 0 or for a non-finite query; any truth value the caller
 * supplies -- nothing is read or written out of bounds for any of them), so
 * sum(conf[i]) + unl[i] == m, and trace(conf[i]) == correct[i] whenever every
 * truth lies in [0, C).  They are defined by the sweep's labels alone, i.e. by
 * the reference's neighbour order and its first-to-strictly-exceed vote
 * (cpp:324-337).
 * Ties: labels equal the reference's at the default "ties" = 1, so conf equals
 * the reference's.  Vote COUNTS depend on which rows are among the k nearest
 * when dist[k-1] == dist[k] (KNN_FLAG_TIE_BOUNDARY): at "ties" = 1 a boundary
 * tie that cannot change the label is ordered by train index, and the counts
 * are those of the rows the call reports (idx); they equal the reference's
 * top-k membership under "ties" = 2.
 *
 * knn_confusion_device: the building block over any label array d_labels
 * [nk][m] (the sweep's layout) and d_truth [m]; needs no train set.  It ADDS
 * into d_conf [nk*C*C] and d_unl [nk] (nullable): the caller zeroes them, and
 * two calls into the same buffers give the sum.  1 <= nk <= 4096, class_cnt
 * >= 1.  The histograms are kept in LDS per wave for class_cnt <= 16, per
 * workgroup for class_cnt <= 96, and counted with global atomics beyond.
 * Device pointers; enqueue only. */
int knn_confusion_device(knn_ctx* ctx, const int32_t* d_labels, int32_t nk, int64_t m,
                         const int32_t* d_truth, int32_t class_cnt, int64_t* d_conf,
                         int64_t* d_unl, void* stream);
/* Vote counts (the reference's label_cnt[] after cpp:324-337, predict_proba
 * times k): d_counts [m][class_cnt] (int32), counts[q][c] = #{t < k : label of
 * row entry t == c} over ordered neighbour rows d_idx [m][kmax] with label
 * d_lab[idx - idx_base], as knn_vote_sweep_device reads them.  0 <= k <= kmax
 * (KNN_ERR_ARG names both otherwise).  Entries with idx -1 are skipped, a row
 * without neighbours gives all zeros: a row sums to min(k, its valid
 * entries).  Every cell of d_counts is written.  Enqueue only. */
int knn_vote_counts_device(knn_ctx* ctx, const int64_t* d_idx, int64_t m, int32_t kmax,
                           const int32_t* d_lab, int64_t idx_base, int32_t k, int32_t class_cnt,
                           int32_t* d_counts, void* stream);
/* knn_classify_sweep_excl_device (d_excl NULL: the plain sweep) plus the
 * evaluation at class_cnt = the train set's.  d_truth [m] is required
 * (KNN_ERR_ARG); d_labels [nk*m], d_correct [nk], d_conf [nk*C*C] and d_unl
 * [nk] are each nullable (without d_labels the labels live in the context's
 * workspace).  Zero-or-accumulate: like d_correct in the device sweeps, d_conf
 * and d_unl are ZEROED by the call on its stream and then hold this call's
 * counts alone; to sum several calls, add the results or use
 * knn_confusion_device, which accumulates.  Enqueue only; KNN_ERR_STATE before
 * set_train. */
int knn_classify_sweep_eval_device(knn_ctx* ctx, const double* dQ, int64_t m,
                                   const int64_t* d_excl, const int32_t* ks, int32_t nk,
                                   int32_t metric, int32_t* d_labels, const int32_t* d_truth,
                                   int64_t* d_correct, int64_t* d_conf, int64_t* d_unl,
                                   void* stream);
/* knn_loo_sweep_device plus the evaluation: truth is the rows' own labels.
 * d_labels [nk*rows], d_correct, d_conf, d_unl nullable; zeroed by the call. */
int knn_loo_sweep_eval_device(knn_ctx* ctx, int64_t row0, int64_t rows, const int32_t* ks,
                              int32_t nk, int32_t metric, int32_t* d_labels, int64_t* d_correct,
                              int64_t* d_conf, int64_t* d_unl, void* stream);
/* Host twins (wait for the result).  truth [m] required; out_labels [nk*m],
 * out_correct [nk], out_conf [nk*C*C], out_unl [nk] each nullable. */
int knn_classify_sweep_eval(knn_ctx* ctx, const double* Q, int64_t m, const int32_t* ks,
                            int32_t nk, int32_t metric, int32_t* out_labels, const int32_t* truth,
                            int64_t* out_correct, int64_t* out_conf, int64_t* out_unl);
/* Leave-one-out over all n_train rows in the 16384-row batches of
 * knn_loo_sweep; out_conf / out_unl are summed over the batches on the device.
 * Without out_labels no [nk][n] array exists anywhere: the label workspace is
 * [nk][16384]. */
int knn_loo_sweep_eval(knn_ctx* ctx, const int32_t* ks, int32_t nk, int32_t metric,
                       int32_t* out_labels, int64_t* out_correct, int64_t* out_conf,
                       int64_t* out_unl);

/* ---- K sweep under group exclusion / leave-one-group-out.  Leave-one-out
 * overstates accuracy whenever train rows are not independent (several samples
 * per writer, patient or subject, augmented copies of one image, exact
 * duplicates): the held-out row's siblings stay in the train set and vote for
 * it.  A train set may carry a group id per row, groups[n] (int32, 0 <= id <
 * n_groups; singletons get ids of their own), and a query a group gq.  One
 * rule fixes every output: the result is what knn_classify_sweep returns on a
 * context whose train set is the current one WITH EVERY ROW r, groups[r] ==
 * gq, REMOVED (labels lose the same entries), reported indices mapped back to
 * the full train set.  That covers the label at every K, the neighbour
 * indices, their order and the distances, the flag bits
 * KNN_FLAG_TIE_BOUNDARY | TIE_VOTE | TIE_ORDER | TIE_REF and the rows "ties" =
 * 0 / 1 / 2 re-order: the order among equal distances is the reference's
 * std::sort over the n - c remaining records in row order (cpp:323), another
 * introsort run than the ones over n or n - 1.  KNN_FLAG_EXACT_RESCAN may
 * differ.  gq = -1, or any gq outside [0, n_groups), excludes nothing: that
 * query equals the plain sweep's.  KNN_VOTE_DISTANCE applies as in every sweep.
 * One search at max(ks) + gmax serves a call (gmax: the largest group's
 * size): large groups are served correctly, but through that wide search.
 * K-fold cross-validation (folds of thousands of rows) has a route of its own
 * that masks nothing inside the candidate pass: knn_set_folds / knn_kfold_sweep
 * below, on fold shards.
 *
 * knn_set_groups / knn_set_groups_device attach the ids to the current train
 * set (local rows, [n_train]); the host variant copies them, the device
 * variant borrows the pointer as knn_set_train_device borrows its labels.
 * KNN_ERR_STATE before a train set exists; KNN_ERR_ARG for an id outside [0,
 * n_groups), naming the first such row (checked on the device, with the
 * histogram of group sizes that gives gmax; the call waits for both, as
 * set_train does for its checks) -- no groups are set then.  groups NULL
 * clears them, and so does every knn_set_train*.  knn_get_group_max: gmax, 0
 * when no groups are set. */
int knn_set_groups(knn_ctx* ctx, const int32_t* groups, int32_t n_groups);
int knn_set_groups_device(knn_ctx* ctx, const int32_t* d_groups, int32_t n_groups);
int32_t knn_get_group_max(knn_ctx* ctx);
/* knn_classify_sweep_excl_device with d_qgroup [m] (device, int32: each
 * query's group) in place of d_excl.  d_qgroup NULL = the plain sweep.  With
 * d_qgroup non-NULL: KNN_ERR_STATE when no groups are set, and ks[i] <=
 * n_train - gmax (KNN_ERR_ARG names the offending entry).  Enqueue only, on
 * the stream on_stream (NULL: the context's own), like its siblings. */
int knn_classify_sweep_gexcl_device(knn_ctx* ctx, const double* dQ, int64_t m,
                                    const int32_t* d_qgroup, const int32_t* ks, int32_t nk,
                                    int32_t metric, int32_t* d_labels, const int32_t* d_truth,
                                    int64_t* d_correct, int64_t* d_idx, double* d_dist,
                                    int32_t* d_flags, void* on_stream);
/* Leave-group-out over train rows [row0, row0 + rows) (as
 * knn_loo_sweep_device): query i excludes the group of row row0 + i, and so
 * itself; its truth is its own label.  0 <= ks[i] <= n_train - gmax.
 * Enqueue only. */
int knn_lgo_sweep_device(knn_ctx* ctx, int64_t row0, int64_t rows, const int32_t* ks, int32_t nk,
                         int32_t metric, int32_t* d_labels, int64_t* d_correct, int64_t* d_idx,
                         double* d_dist, int32_t* d_flags, void* on_stream);
/* Host twin over all n_train rows in the 16384-row batches of knn_loo_sweep
 * (waits for the result).  out_conf [nk*C*C] and out_unl [nk] (nullable) are
 * summed over the batches on the device (knn_confusion_device); out_labels
 * [nk][n] is nullable when out_conf is given; out_correct [nk], out_idx /
 * out_dist [n*kmax], out_flags [n] nullable. */
int knn_lgo_sweep(knn_ctx* ctx, const int32_t* ks, int32_t nk, int32_t metric, int32_t* out_labels,
                  int64_t* out_correct, int64_t* out_conf, int64_t* out_unl, int64_t* out_idx,
                  double* out_dist, int32_t* out_flags);

/* ---- F-fold cross-validated K sweep on fold shards.  The standard way to
 * choose K: folds[n] (int32, 0 <= id < n_folds) assigns every train row to a
 * fold, and each row is classified against the rows of all the OTHER folds.
 * One rule fixes every output: for train row r with f = folds[r] the result is
 * what knn_classify_sweep returns for query X[r] on a context whose train set
 * is the current one WITH EVERY ROW OF FOLD f REMOVED (labels lose the same
 * entries), reported indices mapped back to the full train set -- the rule of
 * knn_lgo_sweep with groups = folds.  It covers the label at every K, idx and
 * its order, dist, KNN_FLAG_TIE_BOUNDARY | TIE_VOTE | TIE_ORDER | TIE_REF and
 * the rows "ties" = 0 / 1 / 2 re-order: the order among equal distances is the
 * reference's std::sort over the n - n_f remaining records in row order
 * (cpp:323).  KNN_FLAG_EXACT_RESCAN is outside the contract.
 * KNN_VOTE_DISTANCE applies as in every sweep.
 * How: nothing is masked inside a candidate kernel (that would compute all n^2
 * pairs and discard 1 / F of them).  knn_set_folds gathers the train set
 * stably, fold by fold, into one fold-major fp64 copy and makes every fold's
 * slice the train set of an internal sub-context on the same device
 * (knn_set_train_device; the parent's precision and tuning keys are forwarded,
 * at knn_set_folds and again at every sweep; the vote mode stays with the
 * parent).  Fold f's rows are then searched in the other F - 1 shards
 * (knn_search_partial_device at w = kmax + 1, shards below w rows padded), the
 * lists' local indices are rewritten to original rows -- the gather is stable,
 * so every list stays sorted by (dist, idx) -- and merged at kmax as
 * knn_merge_vote_device does; the sweep tie scan queues the queries whose label
 * at some K the reference's order could change, and those (rare) are re-ordered
 * by the leave-group-out reference-order pass over the parent's rows with the
 * fold as the group (queue and pass are sized on the device: no host wait);
 * the prefix votes read the parent's labels.  (F - 1) / F n^2 pairs in all.
 * Memory: one extra fp64 copy of the train set (n x d x 8 B, plus labels and
 * two int32 per row) and the folds' candidate images, which add up to one
 * more set of the images a context builds.
 * knn_last_candidate_path / knn_last_kernel_name of the context report the
 * last shard search of the last k-fold call.
 *
 * knn_set_folds: folds is a host array [n_train]; 2 <= n_folds <= 64 and every
 * fold non-empty (KNN_ERR_ARG, naming the empty fold); an id outside [0,
 * n_folds) is KNN_ERR_ARG naming the first such row (set_groups' check and
 * histogram kernel) -- no folds are set then.  KNN_ERR_STATE before a train set
 * exists.  NULL clears the folds, and so does every knn_set_train*.  The call
 * waits, as set_train does.  Independent of knn_set_groups: both may be set.
 * knn_get_fold_max: the largest fold's size, 0 when no folds are set. */
int knn_set_folds(knn_ctx* ctx, const int32_t* folds, int32_t n_folds);
int32_t knn_get_fold_max(knn_ctx* ctx);
/* The sweep of one fold's rows into device buffers, in the fold's ascending
 * original-row order (n_f rows): d_labels [nk][n_f] required; d_correct [nk]
 * (nullable, zeroed by the call: #{rows whose label at ks[i] is their own});
 * d_idx / d_dist [n_f * kmax], d_flags [n_f] nullable.  0 <= ks[i] <= n_train -
 * fold_max (KNN_ERR_ARG names the offending entry); KNN_ERR_STATE without
 * folds; KNN_ERR_ARG for a fold outside [0, n_folds).  Works in batches of at
 * most 16384 rows; enqueue only, on the stream on_stream (NULL: the context's
 * own), like its siblings -- the sub-contexts' work included. */
int knn_kfold_sweep_device(knn_ctx* ctx, int32_t fold, const int32_t* ks, int32_t nk,
                           int32_t metric, int32_t* d_labels, int64_t* d_correct, int64_t* d_idx,
                           double* d_dist, int32_t* d_flags, void* on_stream);
/* Host twin over every fold (waits for the result), outputs in TRAIN ROW order:
 * out_labels [nk][n] (nullable when out_conf is given), out_correct [nk] (the
 * F-fold cross-validation count at ks[i], summed over all rows), out_conf
 * [nk*C*C] and out_unl [nk] (summed over the batches on the device,
 * knn_confusion_device's convention), out_idx / out_dist [n*kmax], out_flags
 * [n]: each nullable.  Batches of at most 16384 rows of one fold, so the
 * workspace does not grow with n. */
int knn_kfold_sweep(knn_ctx* ctx, const int32_t* ks, int32_t nk, int32_t metric,
                    int32_t* out_labels, int64_t* out_correct, int64_t* out_conf, int64_t* out_unl,
                    int64_t* out_idx, double* out_dist, int32_t* out_flags);

/* ---- distance-weighted voting: the second hyperparameter of a KNN classifier.
 * The vote mode is state of the context, like the precision:
 *   KNN_VOTE_UNIFORM (default): the reference's first-to-strictly-exceed vote
 *     (cpp:324-337), every behaviour described above;
 *   KNN_VOTE_DISTANCE: each neighbour votes with weight 1 / distance.
 * The rule, for one query with the ordered neighbour row the call itself
 * reports -- idx[t], dist[t] (the fp64 reference distances), l_t = the label of
 * idx[t], t = 0 .. kmax-1; empty slots (idx -1) count nothing.  The label at
 * prefix length K:
 *   z = #{t < K : dist[t] == 0}     (the row is ascending: the first z entries)
 *   if z >= 1:  entries t < z have weight 1.0; entries t >= z do not vote
 *   else:       w_t = 1.0 / dist[t] (IEEE fp64 division, correctly rounded;
 *                                    1 / inf = 0)
 *   S[c] = 0 for every class; best = -inf; label = -1
 *   for t in 0 .. K-1 in row order (voting entries only):
 *       S[l_t] = S[l_t] + w_t       (one fp64 add per entry, in this order)
 *       if S[l_t] > best: best = S[l_t]; label = l_t
 * So exact matches alone decide when there are any (the usual convention);
 * with unit weights the scan IS the reference's vote, and a row with z >= 1
 * gets the uniform label at min(K, z); `best` is always the largest class sum
 * and the label the class that reached it first; K = 0 gives -1, a non-finite
 * query -1 at every K (KNN_FLAG_NONFINITE), a row whose weights are all 0 the
 * label l_0 (the first voting entry always records).  The result is
 * reproducible bit for bit by that sequential loop.  Permuting entries of equal
 * distance inside the prefix changes no class sum (each class's sequence of
 * addends stays the same); the order among equal distances matters only at the
 * membership boundary (dist[K-1] == dist[K]) and when two classes end on
 * exactly equal sums, and there the label is defined on the rows the call
 * reports: the reference's std::sort order with "ties" = 2; with "ties" = 1 the
 * reference's order where the UNIFORM label could depend on it and train-index
 * order elsewhere.  The search, the tie queue, the flags, idx and dist are
 * exactly what KNN_VOTE_UNIFORM produces for the same call.
 * In KNN_VOTE_DISTANCE mode these calls return the rule's labels (correct,
 * conf and unl follow from them): knn_classify*, knn_classify_sweep* (the
 * _excl variant included), knn_loo_sweep*, the four *_eval* calls, and the
 * knn_group_* twins (knn_group_set_vote).  These stay UNIFORM in every mode:
 * knn_vote_sweep_device, knn_vote_counts_device, knn_merge_vote_device and
 * knn_tie_resolve_device (building blocks; the weighted ones are below).
 * knn_set_vote: KNN_ERR_ARG for any other value, the mode is kept. */
#define KNN_VOTE_UNIFORM 0
#define KNN_VOTE_DISTANCE 1
int knn_set_vote(knn_ctx* ctx, int mode);
/* The context's vote mode (-1 for a null context). */
int knn_get_vote(knn_ctx* ctx);
/* knn_vote_sweep_device by distance: its arguments plus d_dist [m][kmax], the
 * rows' distances (ascending; +inf in empty slots).  Always votes by distance,
 * whatever the context's mode.  An entry with idx -1 (or a negative label)
 * does not vote; a row without voting entries gets -1 at every K.  Same
 * argument checks; device pointers except ks; enqueue only. */
int knn_vote_sweep_weighted_device(knn_ctx* ctx, const int64_t* d_idx, const double* d_dist,
                                   int64_t m, int32_t kmax, const int32_t* d_lab,
                                   int64_t idx_base, const int32_t* ks, int32_t nk,
                                   int32_t* d_labels, const int32_t* d_truth, int64_t* d_correct,
                                   void* stream);
/* The weighted twin of knn_vote_counts_device: d_wsum [m][class_cnt] (fp64) =
 * the class sums S of the rule after the first k entries (the z rule applied;
 * predict_proba times the row's total weight), each class summed sequentially
 * in row order.  0 <= k <= kmax; labels outside [0, class_cnt) count nothing;
 * every cell is written, zeros for a row without neighbours.  Enqueue only. */
int knn_vote_weights_device(knn_ctx* ctx, const int64_t* d_idx, const double* d_dist, int64_t m,
                            int32_t kmax, const int32_t* d_lab, int64_t idx_base, int32_t k,
                            int32_t class_cnt, double* d_wsum, void* stream);

/* Train-sharded building block: exact top-w of THIS context's shard for
 * each query, sorted by (dist, global idx), with each neighbour's label.
 * Rows beyond the shard size are padded with dist=+inf, idx=-1, label=-1.
 * Device pointers: d_dist[m*w], d_idx[m*w], d_lab[m*w]. */
int knn_search_partial_device(knn_ctx* ctx, const double* dQ, int64_t m, int32_t w,
                              int32_t metric, double* d_dist, int64_t* d_idx,
                              int32_t* d_lab, void* stream);
/* k-way merge of `parts` sorted lists per query, laid out [parts][m][w]
 * (the layout an all-gather of knn_search_partial outputs produces), then
 * the reference vote over the first k of the merged order, for queries
 * [q0, q0+mq) (a rank's slice; q0=0, mq=m for all).  Outputs are indexed
 * from 0 (row q-q0).  Device pointers; d_out_idx/d_out_dist/d_flags nullable.
 * Within exact distance ties the merged order is (dist, global idx); a query
 * whose label that order could decide (tuning "ties" of ctx: 1 vote-affecting
 * ties, 2 every tie, 0 none) gets KNN_FLAG_TIE_PENDING in d_flags.  A query
 * no shard listed a neighbour for (non-finite) gets label -1,
 * KNN_FLAG_NONFINITE, idx -1, dist NaN; with fewer than k rows in all, the
 * empty slots are idx -1, dist +inf. */
int knn_merge_vote_device(knn_ctx* ctx, const double* d_dist, const int64_t* d_idx,
                          const int32_t* d_lab, int32_t parts, int64_t m, int32_t w, int32_t k,
                          int64_t q0, int64_t mq, int32_t* d_labels, int64_t* d_out_idx,
                          double* d_out_dist, int32_t* d_flags, void* stream);

/* ---- train-sharded reference tie order (cpp:323/366 over the WHOLE train
 * set, whose std::sort order among equal distances depends on every row).
 * For the KNN_FLAG_TIE_PENDING queries of all ranks (rare):
 * 1. every shard: knn_shard_distances_device -- d_out[i][j] = the exact fp64
 *    distance (cpp:33-67 operation order) of shard row j to query
 *    dQ[d_qsel[i]] (d_qsel NULL: query i), [nsel][n_shard];
 * 2. an all-to-all moves each owner's [nsel_r][n_shard] block to it;
 * 3. the owner: knn_tie_resolve_device over d_D = parts blocks in global row
 *    order, block p = [nsel][rows[p]] at offset nsel * (rows[0] + ... +
 *    rows[p-1]) (what the all-to-all delivers), d_lab_all = the labels of all
 *    rows (global order); runs libstdc++'s introsort as the reference does
 *    and the vote, and rewrites output row d_orow[i] of d_labels / d_idx /
 *    d_dist (k per row) / d_flags (TIE_PENDING -> TIE_REF).  parts <= 64,
 *    sum(rows) < 2^31.  Scratch: ~20 B per row per concurrent query. */
int knn_shard_distances_device(knn_ctx* ctx, const double* dQ, const int32_t* d_qsel,
                               int32_t nsel, int32_t metric, double* d_out, void* stream);
int knn_tie_resolve_device(knn_ctx* ctx, const double* d_D, int32_t parts, const int64_t* rows,
                           int32_t nsel, const int32_t* d_lab_all, const int32_t* d_orow,
                           int32_t k, int32_t* d_labels, int64_t* d_idx, double* d_dist,
                           int32_t* d_flags, void* stream);

/* ---- min-max normalisation (replaces cpp:229-306, bit-exact in fp64) -----
 * Transductive, like the reference: per-dimension max/min over the train
 * rows AND every query set, starting from max = -1 / min = 999999
 * (cpp:239-243, strict compares), then x = (x - min)/(max - min) on the
 * dimensions where max - min != 0.
 * knn_minmax_device folds one device set [rows x d] (fp64, row-major) into
 *   d_max/d_min (device, d doubles each); init != 0 starts from -1/999999
 *   (the first set), 0 folds into the current values (later sets, or the
 *   result of an all-reduce over ranks, ≙ MPI_Allreduce cpp:276-277).
 * knn_normalize_device applies the bounds to a device set in place.
 * knn_normalize runs both on host sets in place (sets[i] has rows[i] rows;
 *   e.g. {train, test, val}); out_max/out_min (nullable) receive the bounds. */
int knn_minmax_device(knn_ctx* ctx, const double* d_X, int64_t rows, int32_t d, double* d_max,
                      double* d_min, int32_t init, void* stream);
int knn_normalize_device(knn_ctx* ctx, double* d_X, int64_t rows, int32_t d,
                         const double* d_max, const double* d_min, void* stream);
int knn_normalize(knn_ctx* ctx, double* const* sets, const int64_t* rows, int32_t nsets,
                  int32_t d, double* out_max, double* out_min);

/* ---- the reference's CSV reader on the GPU (replaces cpp:154-222) ---------
 * Values equal the reference reader's, bit for bit, for every file: data
 * tokens are atof's fp64 values, label tokens atoi's.
 * Token rule (getline on '\n', then on ','; one running token counter c over
 * the whole file, rows come from the count, not from line breaks): position p
 * TERMINATES a token iff text[p] == ',', or text[p] == '\n' (or p == bytes,
 * the end of the file) and p > 0 and text[p-1] is neither ',' nor '\n'; the
 * token begins after the previous ',' or '\n', or at 0.  So every segment
 * followed by a comma is a token (possibly empty), a line's last segment only
 * if it is non-empty.  with_label: token c with c % (dim+1) == 0 is
 * labels[c / (dim+1)], any other token data[c - c/(dim+1) - 1]; without
 * labels token c is data[c].  Tokens at c >= rows * (dim [+ 1]) are counted
 * and not stored; cells no token reaches are NOT written (they keep what the
 * caller put there).
 * Conversion tiers.  A device kernel converts every token it can prove
 * correctly rounded: the whole token must match -? D* (. D*)? ([eE] [+-]? D+)?
 * with at least one mantissa digit, at most 19 significant digits and at most
 * 64 bytes; with w its decimal significand and q its decimal exponent, w == 0
 * gives +-0.0, tier 1 (Clinger: w < 2^53, |q| <= 22) is one correctly rounded
 * fp64 multiply or divide of two exact operands, tier 2 (Eisel-Lemire: any
 * other w < 2^64, -342 <= q <= 308) multiplies by a 128-bit truncated power of
 * five and gives up where the truncation could decide the rounding, on
 * subnormal results and on overflow.  Labels: the whole token -? D{1,9}.
 * Every other token -- blanks, '+', a trailing '\r', hex, inf / nan, garbage,
 * the empty token -- is SLOW: the host runs atof / atoi itself on a
 * NUL-terminated copy (knn_csv_read*), or the caller does
 * (knn_csv_parse_device).
 *
 * knn_csv_parse_device: the building block.  d_text [bytes] is the file's
 * text on the device (16-byte aligned).  Enqueues three steps on `on_stream` (a
 * hipStream_t, NULL = the context's stream, like every _device call): the
 * terminators of every KNN_CSV_BLOCK_BYTES block, their exclusive scan, the
 * conversion; it returns without waiting.  d_data [rows*dim] (fp64), d_labels
 * [rows] (required iff with_label), *d_tokens = the file's token count,
 * *d_nslow = the number of slow tokens among the stored ones, d_slow
 * [slow_cap][2] = (c, p) of each: its token index and its terminator's
 * position, in no particular order.  d_nslow keeps counting past slow_cap;
 * entries beyond it are dropped (call again with a larger list).  bytes == 0
 * launches nothing and reports 0 tokens.  KNN_ERR_ARG for dim < 1, rows < 0 or
 * bytes < 0.  Needs no train set. */
int knn_csv_parse_device(knn_ctx* ctx, const char* d_text, int64_t bytes, int32_t dim,
                         int32_t with_label, int64_t rows, double* d_data, int32_t* d_labels,
                         int64_t* d_tokens, int64_t* d_slow, int64_t slow_cap, int64_t* d_nslow,
                         void* on_stream);
/* A CSV file into host arrays data [rows*dim] and labels [rows] (required iff
 * with_label), *tokens = the tokens found; waits for the result.  Reads the
 * file (parallel pread, at most 16 threads), uploads the text, parses it
 * (token rule and tiers above), copies the values back and converts the slow
 * tokens with atof / atoi: the arrays hold exactly what the reference reader
 * leaves in them.  The slow list starts at max(4096, bytes / 64) entries; when
 * more tokens are slow the conversion runs once more with room for all.  A
 * missing or unreadable file is KNN_ERR_ARG with the path in the message. */
int knn_csv_read(knn_ctx* ctx, const char* path, int32_t dim, int32_t with_label, int64_t rows,
                 double* data, int32_t* labels, int64_t* tokens);
/* The same with the values left on the device (d_data, d_labels: device
 * pointers on the context's GPU; same token rule, tiers and values): the slow
 * tokens' host values go up as an (index, value) list that a small kernel
 * scatters.  Runs on the context's stream; complete on return. */
int knn_csv_read_device(knn_ctx* ctx, const char* path, int32_t dim, int32_t with_label,
                        int64_t rows, double* d_data, int32_t* d_labels, int64_t* tokens);
/* Slow tokens of the last knn_csv_read / knn_csv_read_device (-1: none yet). */
int64_t knn_csv_last_slow(knn_ctx* ctx);
/* Host seconds of that call's parts: out_s[0] reading the file, [1] text to
 * the device, [2] the kernels and the slow list's way back, [3] values to the
 * host (0 for knn_csv_read_device), [4] the slow tokens' conversion. */
int knn_csv_last_phases(knn_ctx* ctx, double out_s[5]);

/* Per-phase device timing with HIP events recorded on the stream the
 * kernels run on (off by default).  Phases: 0 = query prep, 1 = candidate
 * kernel (fused MFMA distance + top-R), 2 = merge/re-rank/vote, 3 = exact
 * rescan.  knn_last_phase_ms: the last classify/search call (waits for it;
 * -1 if none).  knn_timing_totals: per-phase sums over every timed call
 * since the last reset, and their number (waits for them); reset != 0
 * starts a new sum.  Recording never makes a call wait.  enable: 0 off, 1
 * every phase (5 events per call), 2 the candidate kernel only (2 events:
 * each event record holds the stream ~6 us, profiles/ab_log.md r5u; the
 * other phases then read -1 / 0).  Behaviour change (round 5): any other
 * value of enable (earlier builds took every non-zero value as "on") is
 * refused with KNN_ERR_ARG and leaves the timing state unchanged. */
#define KNN_PHASE_PREP 0
#define KNN_PHASE_CANDIDATE 1
#define KNN_PHASE_RERANK 2
#define KNN_PHASE_RESCAN 3
int knn_set_timing(knn_ctx* ctx, int enable);
double knn_last_phase_ms(knn_ctx* ctx, int phase);
int knn_timing_totals(knn_ctx* ctx, double out_ms[4], int64_t* calls, int reset);
/* Geometry of the last candidate launch: out[0]=workgroups, out[1]=splits
 * per query tile, out[2]=list entries per lane (R), out[3]=re-rank count C. */
int knn_last_geometry(knn_ctx* ctx, int64_t out[4]);

/* Candidate-pass precision for L2 (the result is the exact fp64 top-k in
 * every mode; this only selects how candidates are found):
 *   AUTO (default): for batches of >= 4096 queries at d <= 256, int8 when
 *         the train set is integer-coded (every value c / 2^s with the
 *         codes of each dimension spanning <= 255, e.g. byte features),
 *         else fp16 (either until a batch of this train set leaves > 1/16
 *         of its queries to the rescan); otherwise bf16x3 (d > 256 on the
 *         streamed kernel);
 *   FP32: v_mfma_f32_32x32x2_f32 on fp32 copies;
 *   BF16X3: q.x as qh.xh + ql.xh + qh.xl on bf16 MFMA
 *           (hi/lo bf16 split of the fp64 values, ~2^-16 relative error);
 *   FP16: q.x on v_mfma_f32_16x16x32_f16 with both operands in fp16 under
 *         power-of-two scales (~2^-10 relative error), d <= 256.
 * The int8 pass (kernel paths 5 and 6) is exact: v_mfma_i32_16x16x64_i8
 * (dims padded to 64) or v_mfma_i32_32x32x32_i8 (dims padded to 32, chosen
 * where that pads fewer dims, e.g. d = 96) on the codes, centred per
 * dimension; a query off the train set's grid or beyond the codes' range
 * goes to the exact rescan.  It has no precision mode of its own (tuning
 * keys "i8", "i8w").
 * L1 (Manhattan) takes the fp32 VALU pass (path 1), except that AUTO runs
 * batches of >= 4096 queries (k <= 63) against an integer-coded train set at
 * d <= 256 on the same int8 codes (kernel path 7: v_sad_u8, four dims per
 * lane per instruction; sums of absolute code differences are the
 * reference's distances times 2^s, exactly), until a batch leaves > 1/16 of
 * its queries to the rescan (queries off the train set's grid or beyond the
 * codes' range go there).  Tuning key "i8l1": 1 at every batch size, 0 never.
 * d > 256 (MNIST's 784 included) stays on the fp32 stream kernel unless
 * "i8l1" = 2 asks for the wide form of the pass, which serves 256 < d <= 1024
 * (opt-in: never AUTO's choice).
 * Any other L1 call at d <= 256 -- real-valued data, byte data after the
 * reference's Normalize = true (x / 255 is on no binary grid) -- can take a
 * lossy-but-certified pass on 16-bit fixed-point codes (kernel path 8:
 * v_sad_u16, two dims per lane per instruction).  Codes are clamp(rint(2^e (v
 * - mean)), -32768, 32767) + 32768 with one power-of-two scale for all
 * dimensions, chosen so the train rows take half the code range; the proxy's
 * error is at most 2^-e times the two vectors' summed coding errors, which
 * the library measures (train rows when the image is built, each query in
 * the merge) and certifies against; a query clamped far outside the train
 * set's range fails certification and goes to the exact rescan.  Results are
 * unchanged.  Tuning key "u16l1": 0 off (the default), 1 on at every batch
 * size; opt-in only, AUTO never chooses it; where "i8l1" selects path 7 for
 * an integer-coded train set, that exact pass wins.
 * The same pass serves 256 < d <= 1024 (the reference's default dim = 784
 * with Normalize = true) in a wide form that re-reads the query codes per
 * train tile (cand_fix16_wide_kernel).  Its integer sums reach 65535 x 1024 <
 * 2^26 and are rounded once to float, off by at most 1 code unit up to 512
 * padded dims and 2 up to 1024; that term is part of the certified bound, so
 * results are unchanged.  Tuning key "u16l1w": 0 off (the default), 1 on at
 * every batch size; opt-in only; "i8l1" = 2 wins for an integer-coded set.
 * Environment override at knn_create: KNN_PRECISION=fp32|bf16x3|fp16. */
#define KNN_PRECISION_AUTO 0
#define KNN_PRECISION_FP32 1
#define KNN_PRECISION_BF16X3 2
#define KNN_PRECISION_FP16 3
int knn_set_precision(knn_ctx* ctx, int mode);
/* Candidate kernel flavour of the last search: 0 fp32 L2, 1 fp32 L1, 2 bf16x3
 * L2 (32x32x16 MFMA), 3 bf16x3 L2 (16x16x32), 4 fp16 L2 (16x16x32), 5 int8
 * L2 (16x16x64, exact integer dot products), 6 int8 L2 (32x32x32), 7 L1 on
 * int8 codes (v_sad_u8, exact integer sums; d <= 256, or <= 1024 with "i8l1"
 * = 2), 8 L1 on 16-bit fixed-point codes (v_sad_u16, certified; d <= 256, or
 * <= 1024 with "u16l1w" = 1). */
int knn_last_candidate_path(knn_ctx* ctx);
/* Name of the last candidate kernel launched, as rocprofv3 reports it
 * without namespace, spaces and argument list (e.g. "cand_kernel<128,4,4,8>"). */
const char* knn_last_kernel_name(knn_ctx* ctx);

/* Tuning overrides for experiments (0 = automatic): "R" list entries per
 * lane (4, 8, 16), "S" train splits per query tile (1..64), "nw" waves per
 * candidate workgroup (4, 8 or 16 where the kernel has the variant), "ablate"
 * (bits 0/1/3/4: timing-only kernel ablations -- no staging, no selection,
 * L2-resident staging, no workgroup barrier -- results invalid; bit 2: no
 * per-query global threshold exchange, results stay exact); -1 = auto for "fp16" (fp16
 * candidate pass: 0 off, 1 on), "i8" (the int8 candidate pass where the
 * train set is integer-coded: 0 off, 1 on at every batch size; L2 only),
 * "i8l1" (the L1 pass on int8 codes, path 7, where the train set is
 * integer-coded and d <= 256: 0 off, 1 on at every batch size, -1 auto; 2: as
 * 1, and also at 256 < d <= 1024 on the wide kernel, cand_sad_wide_kernel --
 * beyond 1024 dims, off the grid or under L2 it plans what 0 plans), "u16l1"
 * (no auto: 0 off, the default; 1 the L1 pass on 16-bit fixed-point codes,
 * path 8, for any train set at d <= 256 and every batch size, except where
 * "i8l1" selects path 7; it moves no L2 call and no call at d > 256), "u16l1w"
 * (no auto: 0 off, the default; 1 that pass at 256 < d <= 1024 on the wide
 * kernel, cand_fix16_wide_kernel, at every batch size, except where "i8l1" =
 * 2 selects path 7; it moves no L2 call and no call at d <= 256), "i8w" (int8
 * kernel: -1 auto, 0 the 16x16x64 one, 1 the 32x32x32 one; also read by
 * knn_set_train*, whose norm blocks interleave the rows over that kernel's
 * lane lists -- set it before the train set: a later change keeps results
 * exact but loses the interleave's certification odds), "mfma16" (bf16x3 on the 16x16x32 layout: 0
 * off, 1 on), "s3q" (the fp16 d > 256 kernel on 16x16x32: 0 off, 1 on), "qres"
 * (1: where "s3q" runs and d pads to 32 x {9, 10, 12, 14, 16, 18, 20, 24,
 * 25, 28, 30}, the query-resident kernel replaces it -- queries held in
 * registers, rows streamed; 0 off: S3; -1 auto) and
 * "gk" (what the global threshold exchange publishes: 0 the lists' R-th
 * entries (resident kernel) / no exchange (S3), K = 1..16 the K-th smallest
 * of a workgroup's union of a query's lists; results stay exact); "ties"
 * (the reference's std::sort order for tied queries: 0 off, 1 (default) the
 * queries whose label it can change, 2 every query with a tie in its top k);
 * "seed" (experiment: seeded global thresholds of the fp16 / int8 resident
 * kernels from a pre-pass over N strided train rows; 0 / -1 off, the
 * default -- measured slower; results stay exact); "order" (region order of
 * the train images, read by knn_set_train*: -1 auto -- on for integer-coded
 * train sets (the int8 pass) whose int8 image (n x (padded d + 16) bytes) is
 * at most 192 MB and for other sets whose fp16 image (n x (2 padded d + 16)
 * bytes) is at most 512 MB, with P = min(64, n / 16384) regions and at
 * least 8 of them -- 0 off, 1 on with P = min(64, n / 16384) regions (stays
 * off below n = 32768, where P < 2), 2..64 that many regions (at most n /
 * 256); queries of the resident fp16 / int8 kernels are then sorted by
 * region and each query tile's stream starts at its region -- "ophase": -1
 * auto (at the first region of its region's eighth of the chain, so 8
 * groups of query tiles share their streams), 0 its own region, N phases);
 * "nblk" (norm blocks of the train images, read by knn_set_train*: every
 * 16384-row window of the image order sorted by the rows' squared norm, so
 * the int8 kernels' per-sub-tile seed bound is tight; -1 auto -- on for
 * integer-coded train sets of more than 16384 rows at d <= 256 -- 0 off, 1
 * on, 2 on as plain sorted windows, 3 on with the interleave only: by
 * default the norm ranks of each 32-row sub-tile are spread over the int8
 * kernel's per-lane lists and the sub-tiles over the window's tiles, so rows
 * of adjacent norm share neither a list nor a split); "s3gq" (the fp16 d > 256 kernel's largest XCD grouping of query
 * tiles, 0 = 4); "xhswz" (the fp16 image's chunk swizzle: 1 on, 0 off);
 * "i8resc" (the fast rescan of failed queries on the train grid filters the
 * int8 32x32x32 kernel's image exactly on the codes: -1 auto = on, 0 every
 * failed query on the fp32 filter);
 * all of them leave results exact. */
int knn_set_tuning(knn_ctx* ctx, const char* key, int64_t value);

/* Synchronise the context's stream. */
int knn_sync(knn_ctx* ctx);
/* Last classify's count of queries that needed the exact rescan (waits for
 * that call; -1 on error). */
int64_t knn_last_rescan_count(knn_ctx* ctx);
/* Rescan counts summed over calls since the last reset: out[0] = queries
 * that failed certification, out[1] = of those, queries finished by the full
 * exact scan.  Waits for the context's work; reset != 0 zeroes the sums. */
int knn_rescan_totals(knn_ctx* ctx, int64_t out[2], int reset);
/* Queries re-ordered as the reference's std::sort orders them
 * (KNN_FLAG_TIE_REF) summed over calls since the last reset.  Waits for the
 * context's work; reset != 0 zeroes the sum. */
int knn_tie_totals(knn_ctx* ctx, int64_t* out, int reset);

/* ---- single-process multi-GPU group over RCCL (xGMI) ---------------------
 * mode 0 = query-sharded: the train set is RCCL-broadcast from device
 *          devs[0] to every GPU (≙ MPI_Bcast cpp:224-225); queries are
 *          split into contiguous shards (≙ MPI_Scatter cpp:226-227, ragged
 *          shards allowed); labels land in one host array (≙ MPI_Gather
 *          cpp:340/383).
 * mode 1 = train-sharded: every GPU holds n/G rows; each computes the exact
 *          local top-(k+1) for all queries; ncclAllGather exchanges the lists;
 *          each GPU k-way merges and votes its slice of the queries; queries
 *          whose label the reference's tie order decides (KNN_FLAG_TIE_PENDING)
 *          get it from an RCCL send/recv exchange of their exact distances
 *          (knn_tie_resolve_device), so every mode gives the same labels.
 * Transport: RCCL whenever G > 1 and the devices are distinct.
 *   | KNN_GROUP_RCCL: RCCL also at G = 1 (a one-rank communicator: every
 *     collective of the path runs through RCCL; env KNN_GROUP_RCCL=1 too).
 *   Repeated devices in devs (e.g. {0, 0, 0}): several ranks share a GPU and
 *     the collectives run as stream-ordered device copies (loopback) -- the
 *     whole G-rank decomposition on fewer GPUs, for tests. */
#define KNN_GROUP_RCCL 0x100
int knn_group_create(knn_group** out, int ndev, const int* devs, int mode);
/* Transport of a group: 0 none (G = 1), 1 RCCL, 2 loopback copies. */
int knn_group_transport(knn_group* g);
/* knn_set_precision / knn_set_tuning on every rank's context. */
int knn_group_set_precision(knn_group* g, int mode);
int knn_group_set_tuning(knn_group* g, const char* key, int64_t value);
/* knn_set_vote on every rank's context.  KNN_VOTE_DISTANCE: in mode 0 each
 * rank's context votes by distance; in mode 1 the weighted vote runs over the
 * merged rows (after the cross-shard tie exchange) with the all-rows label
 * array, so every mode gives the one-context labels.  knn_group_loo_sweep*
 * still refuse mode 1. */
int knn_group_set_vote(knn_group* g, int mode);
int knn_group_destroy(knn_group* g);
int knn_group_set_train(knn_group* g, const double* X, const int32_t* labels, int64_t n,
                        int32_t d, int32_t class_cnt);
int knn_group_classify(knn_group* g, const double* Q, int64_t m, int32_t k, int32_t metric,
                       int32_t* out_labels, int64_t* out_idx, double* out_dist,
                       int32_t* out_flags);
/* K sweep over the group (see knn_classify_sweep): out_labels [nk*m] in host
 * query order, out_correct [nk] summed over the ranks (required iff truth).
 * mode 0: each rank sweeps its query slice.  mode 1: the partial lists and
 * the merge run at kmax, the sweep tie scan fills each rank's tie queue, the
 * cross-shard exchange restores the reference's order, and the prefix votes
 * read the all-rows label array; knn_group_last_tie_count reports the queries
 * the exchange resolved. */
int knn_group_classify_sweep(knn_group* g, const double* Q, int64_t m, const int32_t* ks,
                             int32_t nk, int32_t metric, int32_t* out_labels,
                             const int32_t* truth, int64_t* out_correct);
/* Leave-one-out K sweep over the group (see knn_loo_sweep; cpp:308-343 with
 * the train set as its own validation set): out_labels [nk][n] in train row
 * order, out_correct [nk] (nullable).  mode 0: rank r takes rows [n r / G,
 * n (r + 1) / G) of the train set every rank holds, in batches of at most
 * 16384 rows; the host sums out_correct.  mode 1 (train-sharded): not served,
 * KNN_ERR_ARG with a message saying so. */
int knn_group_loo_sweep(knn_group* g, const int32_t* ks, int32_t nk, int32_t metric,
                        int32_t* out_labels, int64_t* out_correct);
/* The group sweeps with the per-class evaluation (see knn_classify_sweep_eval
 * and knn_loo_sweep_eval): truth [m] required for the classify sweep;
 * out_labels, out_correct, out_conf [nk*C*C] and out_unl [nk] each nullable;
 * every rank evaluates its own slice on its GPU and the host sums conf / unl
 * over the ranks, as it sums out_correct.  knn_group_classify_sweep_eval
 * serves modes 0 and 1; knn_group_loo_sweep_eval serves mode 0 and refuses
 * mode 1 (train-sharded) with the message of knn_group_loo_sweep. */
int knn_group_classify_sweep_eval(knn_group* g, const double* Q, int64_t m, const int32_t* ks,
                                  int32_t nk, int32_t metric, int32_t* out_labels,
                                  const int32_t* truth, int64_t* out_correct, int64_t* out_conf,
                                  int64_t* out_unl);
int knn_group_loo_sweep_eval(knn_group* g, const int32_t* ks, int32_t nk, int32_t metric,
                             int32_t* out_labels, int64_t* out_correct, int64_t* out_conf,
                             int64_t* out_unl);
/* Leave-group-out over the group (see knn_set_groups and knn_lgo_sweep), mode
 * 0 only.  knn_group_set_groups: groups [n] (host; NULL clears) go to every
 * rank's copy of the train set; knn_group_set_train clears them.
 * knn_group_lgo_sweep: rank r takes rows [n r / G, n (r + 1) / G) in batches
 * of at most 16384 rows, as knn_group_loo_sweep; out_labels [nk][n] (nullable
 * when out_conf is given), out_correct, out_conf [nk*C*C], out_unl [nk]
 * nullable, summed over the ranks on the host.  mode 1 (train-sharded): not
 * served by either call, KNN_ERR_ARG with a message saying so. */
int knn_group_set_groups(knn_group* g, const int32_t* groups, int32_t n_groups);
int knn_group_lgo_sweep(knn_group* g, const int32_t* ks, int32_t nk, int32_t metric,
                        int32_t* out_labels, int64_t* out_correct, int64_t* out_conf,
                        int64_t* out_unl);
/* K-fold sweep over the group (see knn_set_folds and knn_kfold_sweep), mode 0
 * only.  knn_group_set_folds: folds [n] (host; NULL clears) go to every rank's
 * copy of the train set, each rank builds the fold shards on its GPU;
 * knn_group_set_train clears them.  knn_group_kfold_sweep: rank r sweeps folds
 * r, r + G, ... (a host thread per rank); out_labels [nk][n] in train row order
 * (nullable when out_conf is given), out_correct, out_conf [nk*C*C], out_unl
 * [nk] nullable, summed over the ranks on the host.  mode 1 (train-sharded):
 * not served by either call, KNN_ERR_ARG with a message saying so. */
int knn_group_set_folds(knn_group* g, const int32_t* folds, int32_t n_folds);
int knn_group_kfold_sweep(knn_group* g, const int32_t* ks, int32_t nk, int32_t metric,
                          int32_t* out_labels, int64_t* out_correct, int64_t* out_conf,
                          int64_t* out_unl);
/* Seconds of the last group classify spent between the first enqueue and
 * the last device completion (device-resident inputs, excludes H2D/D2H). */
double knn_group_last_compute_seconds(knn_group* g);
/* Mode 1: queries of the last classify that took the cross-shard reference
 * tie order (KNN_FLAG_TIE_PENDING -> KNN_FLAG_TIE_REF). */
int64_t knn_group_last_tie_count(knn_group* g);
/* Normalisation over the group (cpp:229-306 with the reference's own
 * decomposition): GPU g takes rows [r*g/G, r*(g+1)/G) of every host set,
 * reduces its max/min, ncclAllReduce MAX/MIN combines them (≙ MPI_Allreduce
 * cpp:276-277), and each GPU rewrites its rows in place. */
int knn_group_normalize(knn_group* g, double* const* sets, const int64_t* rows, int32_t nsets,
                        int32_t d);

#ifdef __cplusplus
}
#endif
#endif /* KNN_AMD_H */
