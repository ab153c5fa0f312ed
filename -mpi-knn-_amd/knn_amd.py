"""Python mirror of the MI355X KNN classifier (ctypes over lib/libknn_amd.so).

The reference (Jason-Woo/-MPI-KNN-, knn_mpi.cpp) has no library API: its
interface is the constant block (cpp:108-119), the CSV formats and the
outputs.  `KnnConfig` carries those constants under the same names;
`Classifier` is the per-GPU hot path (set_train / classify); `run_driver`
reproduces the reference's main() end to end through the native drop-in
driver (bin/knn_mpi_amd) -- the product, not the reference program.

There is no CPU compute path: every call goes through the HIP library and
fails loudly (KnnError) when the library or the GPU is missing.
"""
import ctypes
import dataclasses
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "lib", "libknn_amd.so")
# experiment builds (tools/build_variant.sh) are selected by file name under lib/
if os.environ.get("KNN_AMD_VARIANT"):
    LIB_PATH = os.path.join(HERE, "lib", "libknn_amd_%s.so" % os.environ["KNN_AMD_VARIANT"])
DRIVER_PATH = os.path.join(HERE, "bin", "knn_mpi_amd")

L2, L1 = 0, 1
FLAG_EXACT_RESCAN, FLAG_TIE_BOUNDARY, FLAG_TIE_VOTE, FLAG_TIE_ORDER = 1, 2, 4, 8
FLAG_NONFINITE, FLAG_TIE_REF, FLAG_TIE_PENDING = 16, 32, 64
EXPORTED = (
    "knn_version", "knn_last_error", "knn_device_count", "knn_create", "knn_destroy",
    "knn_set_train", "knn_set_train_device", "knn_classify", "knn_classify_device",
    "knn_search_partial_device", "knn_merge_vote_device", "knn_sync", "knn_last_rescan_count",
    "knn_group_create", "knn_group_destroy", "knn_group_set_train", "knn_group_classify",
    "knn_group_last_compute_seconds", "knn_set_timing", "knn_last_phase_ms",
    "knn_last_geometry", "knn_set_precision", "knn_last_candidate_path", "knn_set_tuning",
    "knn_minmax_device", "knn_normalize_device", "knn_normalize", "knn_group_normalize",
    "knn_timing_totals", "knn_rescan_totals", "knn_last_kernel_name", "knn_tie_totals",
    "knn_shard_distances_device", "knn_tie_resolve_device", "knn_group_transport",
    "knn_group_last_tie_count", "knn_group_set_precision", "knn_group_set_tuning",
    "knn_vote_sweep_device", "knn_classify_sweep_device", "knn_classify_sweep",
    "knn_group_classify_sweep", "knn_classify_sweep_excl_device", "knn_loo_sweep_device",
    "knn_loo_sweep", "knn_group_loo_sweep",
    "knn_confusion_device", "knn_vote_counts_device", "knn_classify_sweep_eval_device",
    "knn_loo_sweep_eval_device", "knn_classify_sweep_eval", "knn_loo_sweep_eval",
    "knn_group_classify_sweep_eval", "knn_group_loo_sweep_eval",
    "knn_set_vote", "knn_get_vote", "knn_group_set_vote", "knn_vote_sweep_weighted_device",
    "knn_vote_weights_device",
    "knn_set_groups", "knn_set_groups_device", "knn_get_group_max",
    "knn_classify_sweep_gexcl_device", "knn_lgo_sweep_device", "knn_lgo_sweep",
    "knn_group_set_groups", "knn_group_lgo_sweep",
    "knn_set_folds", "knn_get_fold_max", "knn_kfold_sweep_device", "knn_kfold_sweep",
    "knn_group_set_folds", "knn_group_kfold_sweep",
    "knn_csv_parse_device", "knn_csv_read", "knn_csv_read_device", "knn_csv_last_slow",
    "knn_csv_last_phases",
)
# bytes of CSV text one workgroup of knn_csv_parse_device owns (knn_amd.h)
CSV_BLOCK_BYTES = 16384
# knn_confusion_device keeps its histograms in LDS per wave up to CONF_SMALL_C
# classes, per workgroup up to CONF_LDS_C, and counts with global atomics
# beyond; knn_vote_counts_device keeps LDS counters up to COUNTS_LDS_C classes
CONF_SMALL_C, CONF_LDS_C, COUNTS_LDS_C = 16, 96, 1024
GROUP_RCCL = 0x100  # knn_group_create mode flag: RCCL collectives also at one GPU
TRANSPORT_NONE, TRANSPORT_RCCL, TRANSPORT_LOOPBACK = 0, 1, 2
PRECISION_AUTO, PRECISION_FP32, PRECISION_BF16X3, PRECISION_FP16 = 0, 1, 2, 3
PHASE_PREP, PHASE_CANDIDATE, PHASE_RERANK, PHASE_RESCAN = 0, 1, 2, 3
# vote mode of a context (knn_set_vote): the reference's unweighted vote, or
# weight 1 / distance with exact matches deciding alone (knn_amd.h)
VOTE_UNIFORM, VOTE_DISTANCE = 0, 1


class KnnError(RuntimeError):
    pass


@dataclasses.dataclass
class KnnConfig:
    """The reference's configuration constants (cpp:108-119), same defaults."""
    dim: int = 784
    K: int = 50
    N_train: int = 60000
    N_test: int = 10000
    N_val: int = 10000
    class_cnt: int = 10
    Euclidean_distance: bool = True
    Normalize: bool = True
    Validation: bool = True
    train_file_name: str = "mnist_train.csv"
    validation_file_name: str = "mnist_validation.csv"
    test_file_name: str = "mnist_test.csv"


def build(jobs=8):
    subprocess.run(["make", "-s", "-j%d" % jobs, "-C", HERE], check=True)


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise KnnError("HIP library not built: %s (run build())" % LIB_PATH)
    # PyTorch-ROCm bundles its own HIP/HSA runtime with the same sonames as
    # /opt/rocm's.  If torch is in the process, let it bring up its runtime
    # first so this library binds to the already-loaded one (two runtimes in
    # one process leave torch without devices).
    if "torch" in sys.modules:
        try:
            sys.modules["torch"].cuda.init()
        except Exception:
            pass
    L = ctypes.CDLL(LIB_PATH)
    P, i32, i64, f64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_double
    sig = {
        "knn_version": ([], ctypes.c_char_p),
        "knn_last_error": ([], ctypes.c_char_p),
        "knn_device_count": ([], ctypes.c_int),
        "knn_create": ([ctypes.POINTER(P), ctypes.c_int], ctypes.c_int),
        "knn_destroy": ([P], ctypes.c_int),
        "knn_set_train": ([P, P, P, i64, i32, i32], ctypes.c_int),
        "knn_set_train_device": ([P, P, P, i64, i32, i32, i64], ctypes.c_int),
        "knn_classify": ([P, P, i64, i32, i32, P, P, P, P], ctypes.c_int),
        "knn_classify_device": ([P, P, i64, i32, i32, P, P, P, P, P], ctypes.c_int),
        "knn_search_partial_device": ([P, P, i64, i32, i32, P, P, P, P], ctypes.c_int),
        "knn_merge_vote_device": ([P, P, P, P, i32, i64, i32, i32, i64, i64, P, P, P, P, P],
                                  ctypes.c_int),
        "knn_sync": ([P], ctypes.c_int),
        "knn_last_rescan_count": ([P], i64),
        "knn_group_create": ([ctypes.POINTER(P), ctypes.c_int, P, ctypes.c_int], ctypes.c_int),
        "knn_group_destroy": ([P], ctypes.c_int),
        "knn_group_set_train": ([P, P, P, i64, i32, i32], ctypes.c_int),
        "knn_group_classify": ([P, P, i64, i32, i32, P, P, P, P], ctypes.c_int),
        "knn_group_last_compute_seconds": ([P], f64),
        "knn_set_timing": ([P, ctypes.c_int], ctypes.c_int),
        "knn_last_phase_ms": ([P, ctypes.c_int], f64),
        "knn_last_geometry": ([P, ctypes.POINTER(i64)], ctypes.c_int),
        "knn_set_precision": ([P, ctypes.c_int], ctypes.c_int),
        "knn_last_candidate_path": ([P], ctypes.c_int),
        "knn_set_tuning": ([P, ctypes.c_char_p, i64], ctypes.c_int),
        "knn_minmax_device": ([P, P, i64, i32, P, P, i32, P], ctypes.c_int),
        "knn_normalize_device": ([P, P, i64, i32, P, P, P], ctypes.c_int),
        "knn_normalize": ([P, P, P, i32, i32, P, P], ctypes.c_int),
        "knn_group_normalize": ([P, P, P, i32, i32], ctypes.c_int),
        "knn_timing_totals": ([P, ctypes.POINTER(f64), ctypes.POINTER(i64), ctypes.c_int],
                              ctypes.c_int),
        "knn_rescan_totals": ([P, ctypes.POINTER(i64), ctypes.c_int], ctypes.c_int),
        "knn_last_kernel_name": ([P], ctypes.c_char_p),
        "knn_tie_totals": ([P, ctypes.POINTER(i64), ctypes.c_int], ctypes.c_int),
        "knn_shard_distances_device": ([P, P, P, i32, i32, P, P], ctypes.c_int),
        "knn_tie_resolve_device": ([P, P, i32, ctypes.POINTER(i64), i32, P, P, i32, P, P, P, P,
                                    P], ctypes.c_int),
        "knn_group_transport": ([P], ctypes.c_int),
        "knn_group_last_tie_count": ([P], i64),
        "knn_group_set_precision": ([P, ctypes.c_int], ctypes.c_int),
        "knn_group_set_tuning": ([P, ctypes.c_char_p, i64], ctypes.c_int),
        "knn_vote_sweep_device": ([P, P, i64, i32, P, i64, P, i32, P, P, P, P], ctypes.c_int),
        "knn_classify_sweep_device": ([P, P, i64, P, i32, i32, P, P, P, P, P, P, P],
                                      ctypes.c_int),
        "knn_classify_sweep": ([P, P, i64, P, i32, i32, P, P, P, P, P, P], ctypes.c_int),
        "knn_group_classify_sweep": ([P, P, i64, P, i32, i32, P, P, P], ctypes.c_int),
        "knn_classify_sweep_excl_device": ([P, P, i64, P, P, i32, i32, P, P, P, P, P, P, P],
                                           ctypes.c_int),
        "knn_loo_sweep_device": ([P, i64, i64, P, i32, i32, P, P, P, P, P, P], ctypes.c_int),
        "knn_loo_sweep": ([P, P, i32, i32, P, P, P, P, P], ctypes.c_int),
        "knn_group_loo_sweep": ([P, P, i32, i32, P, P], ctypes.c_int),
        "knn_confusion_device": ([P, P, i32, i64, P, i32, P, P, P], ctypes.c_int),
        "knn_vote_counts_device": ([P, P, i64, i32, P, i64, i32, i32, P, P], ctypes.c_int),
        "knn_classify_sweep_eval_device": ([P, P, i64, P, P, i32, i32, P, P, P, P, P, P],
                                           ctypes.c_int),
        "knn_loo_sweep_eval_device": ([P, i64, i64, P, i32, i32, P, P, P, P, P], ctypes.c_int),
        "knn_classify_sweep_eval": ([P, P, i64, P, i32, i32, P, P, P, P, P], ctypes.c_int),
        "knn_loo_sweep_eval": ([P, P, i32, i32, P, P, P, P], ctypes.c_int),
        "knn_group_classify_sweep_eval": ([P, P, i64, P, i32, i32, P, P, P, P, P], ctypes.c_int),
        "knn_group_loo_sweep_eval": ([P, P, i32, i32, P, P, P, P], ctypes.c_int),
        "knn_set_vote": ([P, ctypes.c_int], ctypes.c_int),
        "knn_get_vote": ([P], ctypes.c_int),
        "knn_group_set_vote": ([P, ctypes.c_int], ctypes.c_int),
        "knn_vote_sweep_weighted_device": ([P, P, P, i64, i32, P, i64, P, i32, P, P, P, P],
                                           ctypes.c_int),
        "knn_vote_weights_device": ([P, P, P, i64, i32, P, i64, i32, i32, P, P], ctypes.c_int),
        "knn_set_groups": ([P, P, i32], ctypes.c_int),
        "knn_set_groups_device": ([P, P, i32], ctypes.c_int),
        "knn_get_group_max": ([P], i32),
        "knn_classify_sweep_gexcl_device": ([P, P, i64, P, P, i32, i32, P, P, P, P, P, P, P],
                                            ctypes.c_int),
        "knn_lgo_sweep_device": ([P, i64, i64, P, i32, i32, P, P, P, P, P, P], ctypes.c_int),
        "knn_lgo_sweep": ([P, P, i32, i32, P, P, P, P, P, P, P], ctypes.c_int),
        "knn_group_set_groups": ([P, P, i32], ctypes.c_int),
        "knn_group_lgo_sweep": ([P, P, i32, i32, P, P, P, P], ctypes.c_int),
        "knn_set_folds": ([P, P, i32], ctypes.c_int),
        "knn_get_fold_max": ([P], i32),
        "knn_kfold_sweep_device": ([P, i32, P, i32, i32, P, P, P, P, P, P], ctypes.c_int),
        "knn_kfold_sweep": ([P, P, i32, i32, P, P, P, P, P, P, P], ctypes.c_int),
        "knn_group_set_folds": ([P, P, i32], ctypes.c_int),
        "knn_group_kfold_sweep": ([P, P, i32, i32, P, P, P, P], ctypes.c_int),
        "knn_csv_parse_device": ([P, P, i64, i32, i32, i64, P, P, P, P, i64, P, P], ctypes.c_int),
        "knn_csv_read": ([P, ctypes.c_char_p, i32, i32, i64, P, P, P], ctypes.c_int),
        "knn_csv_read_device": ([P, ctypes.c_char_p, i32, i32, i64, P, P, P], ctypes.c_int),
        "knn_csv_last_slow": ([P], i64),
        "knn_csv_last_phases": ([P, ctypes.POINTER(f64)], ctypes.c_int),
    }
    for name, (args, res) in sig.items():
        fn = getattr(L, name)
        fn.argtypes = args
        fn.restype = res
    _lib = L
    return L


def _check(rc):
    if rc != 0:
        raise KnnError("knn error %d: %s" % (rc, lib().knn_last_error().decode()))


def _ptr(a):
    return None if a is None else a.ctypes.data


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _set_arrays(sets):
    """Host sets (C-contiguous float64 [rows, d], normalised in place) ->
    (pointer array, rows array, nsets, d)."""
    sets = [s for s in sets if s is not None]
    if not sets:
        raise ValueError("no sets")
    d = sets[0].shape[1]
    for s in sets:
        if s.dtype != np.float64 or not s.flags["C_CONTIGUOUS"] or s.ndim != 2 or s.shape[1] != d:
            raise ValueError("sets must be C-contiguous float64 [rows, %d] arrays" % d)
    ptrs = (ctypes.c_void_p * len(sets))(*[s.ctypes.data for s in sets])
    rows = (ctypes.c_int64 * len(sets))(*[s.shape[0] for s in sets])
    return ptrs, rows, len(sets), d


class Classifier:
    """One GPU (≙ one MPI rank).  set_train ≙ MPI_Bcast of Data_train
    (cpp:224-225); classify ≙ the query loop cpp:358-381."""

    def __init__(self, device=0):
        self._h = ctypes.c_void_p()
        _check(lib().knn_create(ctypes.byref(self._h), device))
        self.device = device
        self.n_train = 0
        self.dim = 0
        self.class_cnt = 0

    def close(self):
        if self._h:
            lib().knn_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def set_train(self, X, labels, class_cnt):
        X = _f64(X)
        labels = np.ascontiguousarray(labels, dtype=np.int32)
        n, d = X.shape
        _check(lib().knn_set_train(self._h, _ptr(X), _ptr(labels), n, d, int(class_cnt)))
        self.n_train, self.dim, self.class_cnt = n, d, int(class_cnt)
        self._keep = None
        self._lab = (labels, None, 0)  # (host labels, device pointer, idx_offset) for the counts

    def set_train_device(self, dX_ptr, dlab_ptr, n, d, class_cnt, idx_offset=0, keep=None):
        """Device pointers (e.g. torch tensors' data_ptr()); `keep` holds the
        owning objects alive for the library (the pointers are borrowed)."""
        _check(lib().knn_set_train_device(self._h, dX_ptr, dlab_ptr, n, d, int(class_cnt),
                                          int(idx_offset)))
        self.n_train, self.dim, self.class_cnt = n, d, int(class_cnt)
        self._keep = keep
        self._lab = (None, dlab_ptr, int(idx_offset))

    def classify(self, Q, k, metric=L2, return_neighbors=False, return_counts=False,
                 return_weights=False):
        """Returns labels (int32[m]) and, if requested, (idx[m,k], dist[m,k], flags[m]).
        return_counts appends counts int32[m, class_cnt]: how many of the k
        reported neighbours carry each label (knn_vote_counts_device over the
        rows the call reports; staged through torch device tensors).
        return_weights appends wsum float64[m, class_cnt]: the class sums of
        the distance-weighted vote over the same rows (knn_vote_weights_device;
        in any vote mode)."""
        Q = _f64(Q)
        m = Q.shape[0]
        labels = np.empty(m, np.int32)
        flags = np.empty(m, np.int32)
        rows = return_neighbors or return_counts or return_weights
        idx = np.empty((m, max(k, 1)), np.int64) if rows else None
        dist = (np.empty((m, max(k, 1)), np.float64) if return_neighbors or return_weights
                else None)
        _check(lib().knn_classify(self._h, _ptr(Q), m, int(k), int(metric), _ptr(labels),
                                  _ptr(idx), _ptr(dist), _ptr(flags)))
        out = (labels,)
        if return_neighbors:
            out += (idx[:, :k], dist[:, :k], flags)
        if return_counts:
            out += (self._counts_of(idx, int(k)),)
        if return_weights:
            out += (self._weights_of(idx, dist, int(k)),)
        return out[0] if len(out) == 1 else out

    def _weights_of(self, idx, dist, k):
        import torch
        if self.class_cnt <= 0:
            raise KnnError("vote weights before set_train")
        dev = torch.device("cuda", self.device)
        m, kmax = idx.shape
        host_lab, dlab_ptr, base = self._lab
        dI = torch.from_numpy(idx).to(dev)
        dD = torch.from_numpy(dist).to(dev)
        dL = torch.tensor(host_lab).to(dev) if host_lab is not None else None
        dW = torch.empty((m, self.class_cnt), dtype=torch.float64, device=dev)
        torch.cuda.synchronize(dev)  # the context's stream is not torch's
        self.vote_weights_device(dI.data_ptr(), dD.data_ptr(), m, kmax,
                                 dlab_ptr if dL is None else dL.data_ptr(), k, self.class_cnt,
                                 dW.data_ptr(), idx_base=base)
        self.sync()
        return dW.cpu().numpy()

    def _counts_of(self, idx, k):
        import torch
        if self.class_cnt <= 0:
            raise KnnError("vote counts before set_train")
        dev = torch.device("cuda", self.device)
        m, kmax = idx.shape
        host_lab, dlab_ptr, base = self._lab
        dI = torch.from_numpy(idx).to(dev)
        dL = torch.tensor(host_lab).to(dev) if host_lab is not None else None
        dC = torch.empty((m, self.class_cnt), dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)  # the context's stream is not torch's
        self.vote_counts_device(dI.data_ptr(), m, kmax, dlab_ptr if dL is None else dL.data_ptr(),
                                k, self.class_cnt, dC.data_ptr(), idx_base=base)
        self.sync()
        return dC.cpu().numpy()

    def classify_sweep(self, Q, ks, metric=L2, truth=None, return_neighbors=False, exclude=None,
                       confusion=False, exclude_group=None):
        """Labels for every K of `ks` (any order, duplicates allowed) from one
        search at max(ks): labels int32[nk, m], row i for ks[i].  With `truth`
        (int32[m]) also correct int64[nk] = (labels[i] == truth).sum().  With
        return_neighbors also (idx[m, kmax], dist[m, kmax], flags[m]).
        `exclude` (int64[m], global train indices, -1 = none): query i is
        answered as if train row exclude[i] were not in the train set
        (knn_classify_sweep_excl_device; staged through torch device tensors);
        then every K <= n_train - 1.
        `exclude_group` (int32[m], group ids as in set_groups; -1 or any id no
        row carries = none; not together with `exclude`): query i is answered
        as if no train row of group exclude_group[i] were in the train set
        (knn_classify_sweep_gexcl_device); then every K <= n_train - group_max().
        confusion=True (needs `truth`; not with return_neighbors) appends conf
        int64[nk, C, C] (row = true class, column = predicted) and unl
        int64[nk] (queries whose label or truth is outside [0, C)):
        returns (labels, correct, conf, unl)."""
        Q = _f64(Q)
        m = Q.shape[0]
        ks = np.ascontiguousarray(ks, dtype=np.int32).reshape(-1)
        nk = ks.shape[0]
        kmax = int(ks.max()) if nk else 0
        if truth is not None:
            truth = np.ascontiguousarray(truth, dtype=np.int32)
            if truth.shape != (m,):
                raise ValueError("truth must have one label per query")
        if exclude_group is not None:
            if exclude is not None:
                raise ValueError("exclude and exclude_group are mutually exclusive")
            qg = np.ascontiguousarray(exclude_group, dtype=np.int32)
            if qg.shape != (m,):
                raise ValueError("exclude_group must have one group id (or -1) per query")
            if confusion and (truth is None or return_neighbors):
                raise ValueError("confusion needs truth and excludes return_neighbors")
            return self._sweep_gexcl(Q, qg, ks, kmax, metric, truth, return_neighbors, confusion)
        if exclude is not None:
            exclude = np.ascontiguousarray(exclude, dtype=np.int64)
            if exclude.shape != (m,):
                raise ValueError("exclude must have one train index (or -1) per query")
            if confusion:
                if truth is None or return_neighbors:
                    raise ValueError("confusion needs truth and excludes return_neighbors")
                return self._sweep_eval_excl(Q, exclude, ks, metric, truth)
            return self._sweep_excl(Q, exclude, ks, kmax, metric, truth, return_neighbors)
        if confusion:
            if truth is None or return_neighbors:
                raise ValueError("confusion needs truth and excludes return_neighbors")
            C = self.class_cnt
            labels = np.empty((nk, m), np.int32)
            correct = np.zeros(nk, np.int64)
            conf = np.zeros((nk, C, C), np.int64)
            unl = np.zeros(nk, np.int64)
            _check(lib().knn_classify_sweep_eval(self._h, _ptr(Q), m, _ptr(ks), nk, int(metric),
                                                 _ptr(labels), _ptr(truth), _ptr(correct),
                                                 _ptr(conf), _ptr(unl)))
            return labels, correct, conf, unl
        labels = np.empty((nk, m), np.int32)
        flags = np.empty(m, np.int32)
        idx = np.empty((m, max(kmax, 1)), np.int64) if return_neighbors else None
        dist = np.empty((m, max(kmax, 1)), np.float64) if return_neighbors else None
        correct = np.zeros(nk, np.int64) if truth is not None else None
        _check(lib().knn_classify_sweep(self._h, _ptr(Q), m, _ptr(ks), nk, int(metric),
                                        _ptr(labels), _ptr(truth), _ptr(correct), _ptr(idx),
                                        _ptr(dist), _ptr(flags)))
        out = (labels,) if truth is None else (labels, correct)
        if return_neighbors:
            out += (idx[:, :kmax], dist[:, :kmax], flags)
        return out[0] if len(out) == 1 else out

    def _sweep_excl(self, Q, exclude, ks, kmax, metric, truth, return_neighbors):
        import torch
        dev = torch.device("cuda", self.device)
        m, nk = Q.shape[0], ks.shape[0]
        dQ = torch.from_numpy(Q).to(dev)
        dE = torch.from_numpy(exclude).to(dev)
        dT = torch.from_numpy(truth).to(dev) if truth is not None else None
        dL = torch.empty((nk, m), dtype=torch.int32, device=dev)
        dC = torch.zeros(nk, dtype=torch.int64, device=dev) if truth is not None else None
        dF = torch.empty(m, dtype=torch.int32, device=dev)
        dI = torch.empty((m, max(kmax, 1)), dtype=torch.int64, device=dev) if return_neighbors else None
        dD = torch.empty((m, max(kmax, 1)), dtype=torch.float64, device=dev) if return_neighbors else None
        torch.cuda.synchronize(dev)  # the context's stream is not torch's
        p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        self.classify_sweep_device(p(dQ), m, ks, metric, p(dL), p(dT), p(dC), p(dI), p(dD), p(dF),
                                   d_excl=p(dE))
        self.sync()
        out = (dL.cpu().numpy(),)
        if truth is not None:
            out += (dC.cpu().numpy(),)
        if return_neighbors:
            out += (dI.cpu().numpy()[:, :kmax], dD.cpu().numpy()[:, :kmax], dF.cpu().numpy())
        return out[0] if len(out) == 1 else out

    def _sweep_gexcl(self, Q, qgroup, ks, kmax, metric, truth, return_neighbors, confusion):
        import torch
        dev = torch.device("cuda", self.device)
        m, nk, C = Q.shape[0], ks.shape[0], self.class_cnt
        dQ = torch.from_numpy(Q).to(dev)
        dG = torch.from_numpy(qgroup).to(dev)
        dT = torch.from_numpy(truth).to(dev) if truth is not None else None
        dL = torch.empty((nk, m), dtype=torch.int32, device=dev)
        dC = torch.zeros(nk, dtype=torch.int64, device=dev) if truth is not None else None
        dF = torch.empty(m, dtype=torch.int32, device=dev)
        dI = torch.empty((m, max(kmax, 1)), dtype=torch.int64, device=dev) if return_neighbors else None
        dD = torch.empty((m, max(kmax, 1)), dtype=torch.float64, device=dev) if return_neighbors else None
        dM = torch.zeros((nk, C, C), dtype=torch.int64, device=dev) if confusion else None
        dU = torch.zeros(nk, dtype=torch.int64, device=dev) if confusion else None
        torch.cuda.synchronize(dev)  # the context's stream is not torch's
        p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        self.classify_sweep_gexcl_device(p(dQ), m, p(dG), ks, metric, p(dL), p(dT), p(dC), p(dI),
                                         p(dD), p(dF))
        if confusion:  # on the context's stream, after the sweep
            self.confusion_device(p(dL), nk, m, p(dT), C, p(dM), p(dU))
        self.sync()
        out = (dL.cpu().numpy(),)
        if truth is not None:
            out += (dC.cpu().numpy(),)
        if confusion:
            out += (dM.cpu().numpy(), dU.cpu().numpy())
        if return_neighbors:
            out += (dI.cpu().numpy()[:, :kmax], dD.cpu().numpy()[:, :kmax], dF.cpu().numpy())
        return out[0] if len(out) == 1 else out

    def _sweep_eval_excl(self, Q, exclude, ks, metric, truth):
        import torch
        dev = torch.device("cuda", self.device)
        m, nk, C = Q.shape[0], ks.shape[0], self.class_cnt
        dQ = torch.from_numpy(Q).to(dev)
        dE = torch.from_numpy(exclude).to(dev)
        dT = torch.from_numpy(truth).to(dev)
        dL = torch.empty((nk, m), dtype=torch.int32, device=dev)
        dC = torch.empty(nk, dtype=torch.int64, device=dev)
        dF = torch.empty((nk, C, C), dtype=torch.int64, device=dev)
        dU = torch.empty(nk, dtype=torch.int64, device=dev)
        torch.cuda.synchronize(dev)  # the context's stream is not torch's
        self.classify_sweep_eval_device(dQ.data_ptr(), m, ks, metric, dT.data_ptr(),
                                        d_labels=dL.data_ptr(), d_correct=dC.data_ptr(),
                                        d_conf=dF.data_ptr(), d_unl=dU.data_ptr(),
                                        d_excl=dE.data_ptr())
        self.sync()
        return dL.cpu().numpy(), dC.cpu().numpy(), dF.cpu().numpy(), dU.cpu().numpy()

    def classify_sweep_eval_device(self, dQ_ptr, m, ks, metric, d_truth, d_labels=None,
                                   d_correct=None, d_conf=None, d_unl=None, d_excl=None,
                                   stream=None):
        """Device-pointer sweep with the per-class evaluation (enqueue only):
        d_truth [m] required; d_labels [nk][m], d_correct [nk], d_conf
        [nk][C][C] and d_unl [nk] optional, zeroed by the call; d_excl as in
        classify_sweep_device."""
        ks = np.ascontiguousarray(ks, dtype=np.int32).reshape(-1)
        _check(lib().knn_classify_sweep_eval_device(self._h, dQ_ptr, m, d_excl, _ptr(ks),
                                                    ks.shape[0], int(metric), d_labels, d_truth,
                                                    d_correct, d_conf, d_unl, stream))

    def loo_sweep_eval_device(self, row0, rows, ks, metric, d_labels=None, d_correct=None,
                              d_conf=None, d_unl=None, stream=None):
        """loo_sweep_device with the per-class evaluation (truth = the rows'
        own labels); every output optional, zeroed by the call."""
        ks = np.ascontiguousarray(ks, dtype=np.int32).reshape(-1)
        _check(lib().knn_loo_sweep_eval_device(self._h, int(row0), int(rows), _ptr(ks),
                                               ks.shape[0], int(metric), d_labels, d_correct,
                                               d_conf, d_unl, stream))

    def confusion_device(self, d_labels, nk, m, d_truth, class_cnt, d_conf, d_unl=None,
                         stream=None):
        """conf[i][t][p] += #{q : truth[q] == t, labels[i][q] == p} over device
        labels [nk][m] and truth [m]; unl[i] += the queries outside [0,
        class_cnt).  ADDS into d_conf int64[nk][C][C] / d_unl int64[nk]: zero
        them first.  Needs no train set."""
        _check(lib().knn_confusion_device(self._h, d_labels, int(nk), int(m), d_truth,
                                          int(class_cnt), d_conf, d_unl, stream))

    def vote_counts_device(self, d_idx, m, kmax, d_lab, k, class_cnt, d_counts, idx_base=0,
                           stream=None):
        """counts int32[m][class_cnt] of the labels d_lab[idx - idx_base] among
        the first k entries of ordered rows d_idx [m][kmax] (-1 = empty slot)."""
        _check(lib().knn_vote_counts_device(self._h, d_idx, int(m), int(kmax), d_lab,
                                            int(idx_base), int(k), int(class_cnt), d_counts,
                                            stream))

    def vote_sweep_weighted_device(self, d_idx, d_dist, m, kmax, d_lab, ks, d_labels, idx_base=0,
                                   d_truth=None, d_correct=None, stream=None):
        """vote_sweep_device by distance (in any vote mode): d_dist [m][kmax]
        are the rows' ascending distances; weight 1 / distance, exact matches
        alone decide (knn_vote_sweep_weighted_device)."""
        ks = np.ascontiguousarray(ks, dtype=np.int32).reshape(-1)
        _check(lib().knn_vote_sweep_weighted_device(self._h, d_idx, d_dist, m, int(kmax), d_lab,
                                                    int(idx_base), _ptr(ks), ks.shape[0],
                                                    d_labels, d_truth, d_correct, stream))

    def vote_weights_device(self, d_idx, d_dist, m, kmax, d_lab, k, class_cnt, d_wsum, idx_base=0,
                            stream=None):
        """wsum float64[m][class_cnt]: the class sums of the distance-weighted
        vote after the first k entries of ordered rows d_idx / d_dist [m][kmax],
        each class summed in row order (knn_vote_weights_device)."""
        _check(lib().knn_vote_weights_device(self._h, d_idx, d_dist, int(m), int(kmax), d_lab,
                                             int(idx_base), int(k), int(class_cnt), d_wsum,
                                             stream))

    def set_vote(self, mode):
        """VOTE_UNIFORM (default: the reference's vote) or VOTE_DISTANCE:
        classify, classify_sweep (exclude / confusion included) and loo_sweep
        then vote with weight 1 / distance over the rows they report, exact
        matches deciding alone (knn_amd.h).  The search and the reported
        neighbours do not change.  Another value raises KnnError and keeps the
        mode."""
        _check(lib().knn_set_vote(self._h, int(mode)))

    def get_vote(self):
        return int(lib().knn_get_vote(self._h))

    def loo_sweep(self, ks, metric=L2, return_neighbors=False, confusion=False, labels=True):
        """Leave-one-out K sweep over the whole train set (knn_loo_sweep): every
        train row classified against all the OTHER train rows at every K of
        `ks` (each <= n_train - 1).  Returns (labels int32[nk, n], correct
        int64[nk]) and with return_neighbors also (idx[n, kmax], dist[n, kmax],
        flags[n]); accuracy at ks[i] = correct[i] / n.
        confusion=True (not with return_neighbors) appends conf int64[nk, C, C]
        and unl int64[nk]; with labels=False no [nk, n] label array is made
        anywhere and the result is (correct, conf, unl)."""
        ks = np.ascontiguousarray(ks, dtype=np.int32).reshape(-1)
        nk, n = ks.shape[0], self.n_train
        kmax = int(ks.max()) if nk else 0
        if confusion:
            if return_neighbors:
                raise ValueError("confusion excludes return_neighbors")
            C = self.class_cnt
            out_lab = np.empty((nk, n), np.int32) if labels else None
            correct = np.zeros(nk, np.int64)
            conf = np.zeros((nk, C, C), np.int64)
            unl = np.zeros(nk, np.int64)
            _check(lib().knn_loo_sweep_eval(self._h, _ptr(ks), nk, int(metric), _ptr(out_lab),
                                            _ptr(correct), _ptr(conf), _ptr(unl)))
            return (out_lab, correct, conf, unl) if labels else (correct, conf, unl)
        if not labels:
            raise ValueError("labels=False needs confusion=True")
        labels = np.empty((nk, n), np.int32)
        correct = np.zeros(nk, np.int64)
        flags = np.empty(n, np.int32)
        idx = np.empty((n, max(kmax, 1)), np.int64) if return_neighbors else None
        dist = np.empty((n, max(kmax, 1)), np.float64) if return_neighbors else None
        _check(lib().knn_loo_sweep(self._h, _ptr(ks), nk, int(metric), _ptr(labels),
                                   _ptr(correct), _ptr(idx), _ptr(dist), _ptr(flags)))
        if return_neighbors:
            return labels, correct, idx[:, :kmax], dist[:, :kmax], flags
        return labels, correct

    def set_groups(self, groups, n_groups=None):
        """Attaches a group id per train row (int32[n_train], 0 <= id <
        n_groups; n_groups defaults to max id + 1) for exclude_group= and
        lgo_sweep (knn_set_groups); None clears them, and so does set_train.
        An id out of range raises KnnError naming the row."""
        if groups is None:
            _check(lib().knn_set_groups(self._h, None, 0))
            return
        groups = np.ascontiguousarray(groups, dtype=np.int32).reshape(-1)
        if self.n_train and groups.shape[0] != self.n_train:
            raise ValueError("groups must have one id per train row")
        if n_groups is None:
            n_groups = int(groups.max()) + 1 if groups.size else 1
        _check(lib().knn_set_groups(self._h, _ptr(groups), int(n_groups)))

    def set_groups_device(self, d_groups, n_groups, keep=None):
        """Device pointer variant (borrowed; `keep` holds the owning tensor)."""
        _check(lib().knn_set_groups_device(self._h, d_groups, int(n_groups)))
        self._keep_groups = keep

    def group_max(self):
        """Rows of the largest group; 0 when no groups are set."""
        return int(lib().knn_get_group_max(self._h))

    def lgo_sweep(self, ks, metric=L2, return_neighbors=False, confusion=False, labels=True):
        """Leave-one-group-out K sweep over the whole train set (knn_lgo_sweep):
        every train row classified against the train rows of all the OTHER
        groups at every K of `ks` (each <= n_train - group_max()).  Returns as
        loo_sweep: (labels int32[nk, n], correct int64[nk]), with
        confusion=True also conf int64[nk, C, C] and unl int64[nk] (labels=False
        drops the label array), with return_neighbors also (idx[n, kmax],
        dist[n, kmax], flags[n]) at the end."""
        ks = np.ascontiguousarray(ks, dtype=np.int32).reshape(-1)
        nk, n = ks.shape[0], self.n_train
        kmax = int(ks.max()) if nk else 0
        if not labels and not confusion:
            raise ValueError("labels=False needs confusion=True")
        C = self.class_cnt
        out_lab = np.empty((nk, n), np.int32) if labels else None
        correct = np.zeros(nk, np.int64)
        conf = np.zeros((nk, C, C), np.int64) if confusion else None
        unl = np.zeros(nk, np.int64) if confusion else None
        flags = np.empty(n, np.int32) if return_neighbors else None
        idx = np.empty((n, max(kmax, 1)), np.int64) if return_neighbors else None
        dist = np.empty((n, max(kmax, 1)), np.float64) if return_neighbors else None
        _check(lib().knn_lgo_sweep(self._h, _ptr(ks), nk, int(metric), _ptr(out_lab),
                                   _ptr(correct), _ptr(conf), _ptr(unl), _ptr(idx), _ptr(dist),
                                   _ptr(flags)))
        out = (out_lab, correct) if labels else (correct,)
        if confusion:
            out += (conf, unl)
        if return_neighbors:
            out += (idx[:, :kmax], dist[:, :kmax], flags)
        return out

    def set_folds(self, folds, n_folds=None):
        """Assigns every train row to a fold (int32[n_train], 0 <= id < n_folds,
        2 <= n_folds <= 64, every fold non-empty; n_folds defaults to max id +
        1) and builds the fold shards for kfold_sweep (knn_set_folds); None
        clears them, and so does set_train.  An id out of range raises KnnError
        naming the row.  Costs one more fp64 copy of the train set on the GPU."""
        if folds is None:
            _check(lib().knn_set_folds(self._h, None, 0))
            return
        folds = np.ascontiguousarray(folds, dtype=np.int32).reshape(-1)
        if self.n_train and folds.shape[0] != self.n_train:
            raise ValueError("folds must have one id per train row")
        if n_folds is None:
            n_folds = int(folds.max()) + 1 if folds.size else 1
        _check(lib().knn_set_folds(self._h, _ptr(folds), int(n_folds)))

    def fold_max(self):
        """Rows of the largest fold; 0 when no folds are set."""
        return int(lib().knn_get_fold_max(self._h))

    def kfold_sweep(self, ks, metric=L2, return_neighbors=False, confusion=False, labels=True):
        """F-fold cross-validated K sweep (knn_kfold_sweep): every train row
        classified against the rows of all the OTHER folds at every K of `ks`
        (each <= n_train - fold_max()); correct[i] is the cross-validation
        count at ks[i].  Returns as lgo_sweep, in train row order."""
        ks = np.ascontiguousarray(ks, dtype=np.int32).reshape(-1)
        nk, n = ks.shape[0], self.n_train
        kmax = int(ks.max()) if nk else 0
        if not labels and not confusion:
            raise ValueError("labels=False needs confusion=True")
        C = self.class_cnt
        out_lab = np.empty((nk, n), np.int32) if labels else None
        correct = np.zeros(nk, np.int64)
        conf = np.zeros((nk, C, C), np.int64) if confusion else None
        unl = np.zeros(nk, np.int64) if confusion else None
        flags = np.empty(n, np.int32) if return_neighbors else None
        idx = np.empty((n, max(kmax, 1)), np.int64) if return_neighbors else None
        dist = np.empty((n, max(kmax, 1)), np.float64) if return_neighbors else None
        if idx is not None and kmax == 0:
            idx = dist = None
        _check(lib().knn_kfold_sweep(self._h, _ptr(ks), nk, int(metric), _ptr(out_lab),
                                     _ptr(correct), _ptr(conf), _ptr(unl), _ptr(idx), _ptr(dist),
                                     _ptr(flags)))
        out = (out_lab, correct) if labels else (correct,)
        if confusion:
            out += (conf, unl)
        if return_neighbors:
            if idx is None:
                idx, dist = np.empty((n, 0), np.int64), np.empty((n, 0), np.float64)
            out += (idx[:, :kmax], dist[:, :kmax], flags)
        return out

    def kfold_sweep_device(self, fold, ks, metric, d_labels, d_correct=None, d_idx=None,
                           d_dist=None, d_flags=None, stream=None):
        """The sweep of one fold's rows, in the fold's ascending row order, into
        device buffers (enqueue only): d_labels [nk][n_f], d_correct [nk]."""
        ks = np.ascontiguousarray(ks, dtype=np.int32).reshape(-1)
        _check(lib().knn_kfold_sweep_device(self._h, int(fold), _ptr(ks), ks.shape[0],
                                            int(metric), d_labels, d_correct, d_idx, d_dist,
                                            d_flags, stream))

    def lgo_sweep_device(self, row0, rows, ks, metric, d_labels, d_correct=None, d_idx=None,
                         d_dist=None, d_flags=None, stream=None):
        """Leave-group-out sweep of train rows [row0, row0 + rows) into device
        buffers (enqueue only): d_labels [nk][rows], d_correct [nk]."""
        ks = np.ascontiguousarray(ks, dtype=np.int32).reshape(-1)
        _check(lib().knn_lgo_sweep_device(self._h, int(row0), int(rows), _ptr(ks), ks.shape[0],
                                          int(metric), d_labels, d_correct, d_idx, d_dist, d_flags,
                                          stream))

    def classify_sweep_gexcl_device(self, dQ_ptr, m, d_qgroup, ks, metric, d_labels, d_truth=None,
                                    d_correct=None, d_idx=None, d_dist=None, d_flags=None,
                                    stream=None):
        """Device-pointer sweep under group exclusion (enqueue only): d_qgroup
        device int32[m], each query's group (-1 = none); None: the plain sweep."""
        ks = np.ascontiguousarray(ks, dtype=np.int32).reshape(-1)
        _check(lib().knn_classify_sweep_gexcl_device(self._h, dQ_ptr, m, d_qgroup, _ptr(ks),
                                                     ks.shape[0], int(metric), d_labels, d_truth,
                                                     d_correct, d_idx, d_dist, d_flags, stream))

    def loo_sweep_device(self, row0, rows, ks, metric, d_labels, d_correct=None, d_idx=None,
                         d_dist=None, d_flags=None, stream=None):
        """Leave-one-out sweep of train rows [row0, row0 + rows) into device
        buffers (enqueue only): d_labels [nk][rows], d_correct [nk]."""
        ks = np.ascontiguousarray(ks, dtype=np.int32).reshape(-1)
        _check(lib().knn_loo_sweep_device(self._h, int(row0), int(rows), _ptr(ks), ks.shape[0],
                                          int(metric), d_labels, d_correct, d_idx, d_dist, d_flags,
                                          stream))

    def classify_sweep_device(self, dQ_ptr, m, ks, metric, d_labels, d_truth=None,
                              d_correct=None, d_idx=None, d_dist=None, d_flags=None, stream=None,
                              d_excl=None):
        """Device-pointer sweep (enqueue only); ks is a host sequence.  d_excl
        (device int64[m], global train indices, -1 = none): the sweep under
        exclusion (knn_classify_sweep_excl_device)."""
        ks = np.ascontiguousarray(ks, dtype=np.int32).reshape(-1)
        if d_excl is not None:
            _check(lib().knn_classify_sweep_excl_device(self._h, dQ_ptr, m, d_excl, _ptr(ks),
                                                        ks.shape[0], int(metric), d_labels,
                                                        d_truth, d_correct, d_idx, d_dist,
                                                        d_flags, stream))
            return
        _check(lib().knn_classify_sweep_device(self._h, dQ_ptr, m, _ptr(ks), ks.shape[0],
                                               int(metric), d_labels, d_truth, d_correct, d_idx,
                                               d_dist, d_flags, stream))

    def vote_sweep_device(self, d_idx, m, kmax, d_lab, ks, d_labels, idx_base=0, d_truth=None,
                          d_correct=None, stream=None):
        """Prefix votes of ordered neighbour rows d_idx [m][kmax] (device
        pointers; label of an entry = d_lab[idx - idx_base]) at every K of the
        host sequence ks: d_labels [nk][m], d_correct [nk] with d_truth."""
        ks = np.ascontiguousarray(ks, dtype=np.int32).reshape(-1)
        _check(lib().knn_vote_sweep_device(self._h, d_idx, m, int(kmax), d_lab, int(idx_base),
                                           _ptr(ks), ks.shape[0], d_labels, d_truth, d_correct,
                                           stream))

    def classify_device(self, dQ_ptr, m, k, metric, d_labels, d_idx=None, d_dist=None,
                        d_flags=None, stream=None):
        _check(lib().knn_classify_device(self._h, dQ_ptr, m, int(k), int(metric), d_labels, d_idx,
                                         d_dist, d_flags, stream))

    def search_partial_device(self, dQ_ptr, m, w, metric, d_dist, d_idx, d_lab, stream=None):
        _check(lib().knn_search_partial_device(self._h, dQ_ptr, m, int(w), int(metric), d_dist,
                                               d_idx, d_lab, stream))

    def merge_vote_device(self, d_dist, d_idx, d_lab, parts, m, w, k, d_labels, d_out_idx=None,
                          d_out_dist=None, d_flags=None, stream=None, q0=0, mq=None):
        """k-way merge of [parts][m][w] lists + vote for queries [q0, q0+mq)."""
        mq = m - q0 if mq is None else mq
        _check(lib().knn_merge_vote_device(self._h, d_dist, d_idx, d_lab, int(parts), m, int(w),
                                           int(k), int(q0), int(mq), d_labels, d_out_idx,
                                           d_out_dist, d_flags, stream))

    def shard_distances_device(self, dQ_ptr, d_qsel, nsel, metric, d_out, stream=None):
        """Exact fp64 distances of this context's shard rows to nsel queries
        (dQ rows d_qsel[i], or i when d_qsel is None): d_out [nsel][n_shard]."""
        _check(lib().knn_shard_distances_device(self._h, dQ_ptr, d_qsel, int(nsel), int(metric),
                                                d_out, stream))

    def tie_resolve_device(self, d_D, rows, nsel, d_lab_all, d_orow, k, d_labels, d_idx=None,
                           d_dist=None, d_flags=None, stream=None):
        """Reference order (std::sort over the whole train set) for nsel
        queries whose distances to every row are in d_D as len(rows) blocks
        [nsel][rows[p]] in global row order; rewrites output rows d_orow."""
        arr = (ctypes.c_int64 * len(rows))(*[int(r) for r in rows])
        _check(lib().knn_tie_resolve_device(self._h, d_D, len(rows), arr, int(nsel), d_lab_all,
                                            d_orow, int(k), d_labels, d_idx, d_dist, d_flags,
                                            stream))

    def sync(self):
        _check(lib().knn_sync(self._h))

    def last_rescan_count(self):
        """Queries of the last call that failed certification (waits for it)."""
        return int(lib().knn_last_rescan_count(self._h))

    def rescan_totals(self, reset=False):
        """(failed certification, finished by the full exact scan) summed over
        the calls since the last reset (waits for them)."""
        out = (ctypes.c_int64 * 2)()
        _check(lib().knn_rescan_totals(self._h, out, int(bool(reset))))
        return int(out[0]), int(out[1])

    def tie_totals(self, reset=False):
        """Queries re-ordered as the reference's std::sort orders them
        (KNN_FLAG_TIE_REF), summed over calls since the last reset."""
        out = ctypes.c_int64()
        _check(lib().knn_tie_totals(self._h, ctypes.byref(out), int(bool(reset))))
        return int(out.value)

    def timing_totals(self, reset=False):
        """(per-phase ms summed over timed calls since the last reset, calls)."""
        ms = (ctypes.c_double * 4)()
        calls = ctypes.c_int64()
        _check(lib().knn_timing_totals(self._h, ms, ctypes.byref(calls), int(bool(reset))))
        return [float(v) for v in ms], int(calls.value)

    def last_kernel_name(self):
        """Candidate kernel of the last call, rocprofv3-style ("cand_kernel<128,4,4,8>")."""
        return lib().knn_last_kernel_name(self._h).decode()

    def set_precision(self, mode):
        """PRECISION_AUTO (int8 on integer-coded data, else fp16 / bf16x3 by
        shape, knn_amd.h), PRECISION_FP32, PRECISION_BF16X3, PRECISION_FP16.
        Results are the exact fp64 top-k in every mode."""
        _check(lib().knn_set_precision(self._h, int(mode)))

    def set_tuning(self, key, value):
        """Experiment overrides (knn_amd.h, knn_set_tuning): "R", "S", "nw",
        "ablate", "fp16", "mfma16", "i8", "i8w", "i8l1", "u16l1", "u16l1w", "gk", "s3q", "qres", "s3gq",
        "xhswz", "ties", "seed", "order", "ophase", "nblk"; 0 (or -1 where stated) =
        automatic.  "i8l1": L1 searches on the int8 codes of an
        integer-coded train set at d <= 256 (candidate path 7, v_sad_u8; results
        unchanged): 1 at every batch size, 0 never, -1 auto (batches of >= 4096
        queries in PRECISION_AUTO), 2 as 1 and also at 256 < d <= 1024 (the
        wide kernel, cand_sad_wide_kernel; opt-in only).  "u16l1": 1 = L1
        searches at d <= 256 on 16-bit fixed-point codes of any train set
        (candidate path 8, v_sad_u16; certified, results unchanged) at every
        batch size, except where "i8l1" selects path 7; 0 (default) off; no
        auto.  "u16l1w": 1 = the same pass at 256 < d <= 1024 (the wide
        kernel, cand_fix16_wide_kernel; the sums' rounding to float is part of
        the certified bound), except where "i8l1" = 2 selects path 7; 0
        (default) off; no auto; "u16l1" moves no call above 256 dims.
        "order" and "nblk" shape the train layout and are read by
        set_train: "order" -1 = region order only for integer-coded sets whose
        int8 image is <= 192 MB (n / 16384 regions, up to 64, at least 8),
        1 = n / 16384 regions (off below n = 32768); "nblk" -1 = norm blocks
        for integer-coded sets of more than 16384 rows (d <= 256), 1 on, 2 on
        as plain sorted windows, 3 without spreading the sub-tiles over the
        window's tiles."""
        _check(lib().knn_set_tuning(self._h, key.encode(), int(value)))

    def last_candidate_path(self):
        return int(lib().knn_last_candidate_path(self._h))

    def set_timing(self, enable=True, kernel_only=False):
        """HIP-event phase timing (knn_set_timing): every phase, or with
        kernel_only the candidate kernel alone (2 events per call instead of
        5; each event record holds the stream a few microseconds)."""
        _check(lib().knn_set_timing(self._h, 0 if not enable else (2 if kernel_only else 1)))

    def last_phase_ms(self, phase):
        return float(lib().knn_last_phase_ms(self._h, int(phase)))

    def last_geometry(self):
        out = (ctypes.c_int64 * 4)()
        _check(lib().knn_last_geometry(self._h, out))
        return dict(workgroups=out[0], splits=out[1], lists=out[2], rerank=out[3])

    def normalize(self, *sets):
        """Min-max normalisation of host sets in place (cpp:229-306): e.g.
        normalize(train, test, val).  Returns (max, min) per dimension."""
        ptrs, rows, ns, d = _set_arrays(sets)
        mx, mn = np.empty(d), np.empty(d)
        _check(lib().knn_normalize(self._h, ptrs, rows, ns, d, _ptr(mx), _ptr(mn)))
        return mx, mn

    def minmax_device(self, dX_ptr, rows, d, d_max, d_min, init=True, stream=None):
        """Fold a device set into per-dim bounds (init: start at -1/999999)."""
        _check(lib().knn_minmax_device(self._h, dX_ptr, int(rows), int(d), d_max, d_min,
                                       int(bool(init)), stream))

    def normalize_device(self, dX_ptr, rows, d, d_max, d_min, stream=None):
        _check(lib().knn_normalize_device(self._h, dX_ptr, int(rows), int(d), d_max, d_min,
                                          stream))

    def read_csv(self, path, dim, with_label, rows, device=False):
        """One of the reference's CSV files (cpp:154-222) parsed on the GPU:
        (data [rows, dim] float64, labels [rows] int32 or None, tokens found),
        bit for bit what the reference's reader leaves in zeroed arrays.
        device=False: numpy arrays; device=True: torch tensors on the context's
        GPU (zero-initialised), ready for set_train_device / normalize_device /
        classify_device."""
        tokens = ctypes.c_int64(0)
        if device:
            import torch
            dev = torch.device("cuda", self.device)
            data = torch.zeros((int(rows), int(dim)), dtype=torch.float64, device=dev)
            labels = torch.zeros(int(rows), dtype=torch.int32, device=dev) if with_label else None
            torch.cuda.synchronize(dev)  # the zeros, whichever stream made them
            _check(lib().knn_csv_read_device(
                self._h, os.fsencode(path), int(dim), int(bool(with_label)), int(rows),
                data.data_ptr() or None, labels.data_ptr() or None if with_label else None,
                ctypes.byref(tokens)))
        else:
            data = np.zeros((int(rows), int(dim)), np.float64)
            labels = np.zeros(int(rows), np.int32) if with_label else None
            _check(lib().knn_csv_read(self._h, os.fsencode(path), int(dim),
                                      int(bool(with_label)), int(rows), _ptr(data), _ptr(labels),
                                      ctypes.byref(tokens)))
        return data, labels, tokens.value

    def csv_parse_device(self, d_text, nbytes, dim, with_label, rows, d_data, d_labels, d_tokens,
                         d_slow, slow_cap, d_nslow, stream=None):
        """knn_csv_parse_device: device pointers, enqueue only (knn_amd.h)."""
        _check(lib().knn_csv_parse_device(self._h, d_text, int(nbytes), int(dim),
                                          int(bool(with_label)), int(rows), d_data, d_labels,
                                          d_tokens, d_slow, int(slow_cap), d_nslow, stream))

    def csv_last_slow(self):
        """Slow tokens (converted by the host's atof / atoi) of the last read_csv."""
        return lib().knn_csv_last_slow(self._h)

    def csv_last_phases(self):
        """Seconds of the last read_csv: read, h2d, parse, d2h, slow."""
        out = (ctypes.c_double * 5)()
        _check(lib().knn_csv_last_phases(self._h, out))
        return dict(zip(("read", "h2d", "parse", "d2h", "slow"), out))


class Group:
    """Single-process multi-GPU classifier over RCCL (mode 0 query-sharded,
    1 train-sharded); see include/knn_amd.h.  rccl=True runs every
    collective through RCCL even on one GPU; repeated devices (e.g. [0, 0])
    run several ranks on one GPU over loopback copies."""

    def __init__(self, devices, mode=0, rccl=False):
        self._h = ctypes.c_void_p()
        arr = (ctypes.c_int * len(devices))(*devices)
        flags = GROUP_RCCL if rccl else 0
        self.n_train = 0
        self.class_cnt = 0
        _check(lib().knn_group_create(ctypes.byref(self._h), len(devices), arr, int(mode) | flags))

    def transport(self):
        return int(lib().knn_group_transport(self._h))

    def set_precision(self, mode):
        _check(lib().knn_group_set_precision(self._h, int(mode)))

    def set_tuning(self, key, value):
        _check(lib().knn_group_set_tuning(self._h, key.encode(), int(value)))

    def set_vote(self, mode):
        """Classifier.set_vote on every rank (knn_group_set_vote)."""
        _check(lib().knn_group_set_vote(self._h, int(mode)))

    def last_tie_count(self):
        return int(lib().knn_group_last_tie_count(self._h))

    def close(self):
        if self._h:
            lib().knn_group_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_train(self, X, labels, class_cnt):
        X = _f64(X)
        labels = np.ascontiguousarray(labels, dtype=np.int32)
        n, d = X.shape
        _check(lib().knn_group_set_train(self._h, _ptr(X), _ptr(labels), n, d, int(class_cnt)))
        self.n_train = n
        self.class_cnt = int(class_cnt)

    def classify(self, Q, k, metric=L2, return_neighbors=False):
        Q = _f64(Q)
        m = Q.shape[0]
        labels = np.empty(m, np.int32)
        flags = np.empty(m, np.int32)
        idx = np.empty((m, max(k, 1)), np.int64) if return_neighbors else None
        dist = np.empty((m, max(k, 1)), np.float64) if return_neighbors else None
        _check(lib().knn_group_classify(self._h, _ptr(Q), m, int(k), int(metric), _ptr(labels),
                                        _ptr(idx), _ptr(dist), _ptr(flags)))
        if return_neighbors:
            return labels, idx[:, :k], dist[:, :k], flags
        return labels

    def classify_sweep(self, Q, ks, metric=L2, truth=None, confusion=False):
        """Classifier.classify_sweep over the group: labels int32[nk, m], and
        with `truth` also correct int64[nk] (summed over the ranks); with
        confusion=True (needs truth) also conf int64[nk, C, C] and unl
        int64[nk], summed over the ranks."""
        Q = _f64(Q)
        m = Q.shape[0]
        ks = np.ascontiguousarray(ks, dtype=np.int32).reshape(-1)
        nk = ks.shape[0]
        labels = np.empty((nk, m), np.int32)
        if truth is not None:
            truth = np.ascontiguousarray(truth, dtype=np.int32)
            if truth.shape != (m,):
                raise ValueError("truth must have one label per query")
        correct = np.zeros(nk, np.int64) if truth is not None else None
        if confusion:
            if truth is None:
                raise ValueError("confusion needs truth")
            C = self.class_cnt
            conf = np.zeros((nk, C, C), np.int64)
            unl = np.zeros(nk, np.int64)
            _check(lib().knn_group_classify_sweep_eval(self._h, _ptr(Q), m, _ptr(ks), nk,
                                                       int(metric), _ptr(labels), _ptr(truth),
                                                       _ptr(correct), _ptr(conf), _ptr(unl)))
            return labels, correct, conf, unl
        _check(lib().knn_group_classify_sweep(self._h, _ptr(Q), m, _ptr(ks), nk, int(metric),
                                              _ptr(labels), _ptr(truth), _ptr(correct)))
        return labels if truth is None else (labels, correct)

    def loo_sweep(self, ks, metric=L2, confusion=False, labels=True):
        """Classifier.loo_sweep over the group (mode 0; mode 1 raises KnnError):
        labels int32[nk, n] in train row order, correct int64[nk]; with
        confusion=True also conf int64[nk, C, C] and unl int64[nk], and with
        labels=False then (correct, conf, unl) alone."""
        ks = np.ascontiguousarray(ks, dtype=np.int32).reshape(-1)
        nk = ks.shape[0]
        if confusion:
            C = self.class_cnt
            out_lab = np.empty((nk, self.n_train), np.int32) if labels else None
            correct = np.zeros(nk, np.int64)
            conf = np.zeros((nk, C, C), np.int64)
            unl = np.zeros(nk, np.int64)
            _check(lib().knn_group_loo_sweep_eval(self._h, _ptr(ks), nk, int(metric),
                                                  _ptr(out_lab), _ptr(correct), _ptr(conf),
                                                  _ptr(unl)))
            return (out_lab, correct, conf, unl) if labels else (correct, conf, unl)
        if not labels:
            raise ValueError("labels=False needs confusion=True")
        labels = np.empty((nk, self.n_train), np.int32)
        correct = np.zeros(nk, np.int64)
        _check(lib().knn_group_loo_sweep(self._h, _ptr(ks), nk, int(metric), _ptr(labels),
                                         _ptr(correct)))
        return labels, correct

    def set_groups(self, groups, n_groups=None):
        """Classifier.set_groups on every rank (mode 0; mode 1 raises KnnError)."""
        if groups is None:
            _check(lib().knn_group_set_groups(self._h, None, 0))
            return
        groups = np.ascontiguousarray(groups, dtype=np.int32).reshape(-1)
        if self.n_train and groups.shape[0] != self.n_train:
            raise ValueError("groups must have one id per train row")
        if n_groups is None:
            n_groups = int(groups.max()) + 1 if groups.size else 1
        _check(lib().knn_group_set_groups(self._h, _ptr(groups), int(n_groups)))

    def lgo_sweep(self, ks, metric=L2, confusion=False, labels=True):
        """Classifier.lgo_sweep over the group (mode 0; mode 1 raises KnnError):
        the results of loo_sweep, under group exclusion."""
        ks = np.ascontiguousarray(ks, dtype=np.int32).reshape(-1)
        nk = ks.shape[0]
        if not labels and not confusion:
            raise ValueError("labels=False needs confusion=True")
        C = self.class_cnt
        out_lab = np.empty((nk, self.n_train), np.int32) if labels else None
        correct = np.zeros(nk, np.int64)
        conf = np.zeros((nk, C, C), np.int64) if confusion else None
        unl = np.zeros(nk, np.int64) if confusion else None
        _check(lib().knn_group_lgo_sweep(self._h, _ptr(ks), nk, int(metric), _ptr(out_lab),
                                         _ptr(correct), _ptr(conf), _ptr(unl)))
        out = (out_lab, correct) if labels else (correct,)
        return out + (conf, unl) if confusion else out

    def set_folds(self, folds, n_folds=None):
        """Classifier.set_folds on every rank (mode 0; mode 1 raises KnnError)."""
        if folds is None:
            _check(lib().knn_group_set_folds(self._h, None, 0))
            return
        folds = np.ascontiguousarray(folds, dtype=np.int32).reshape(-1)
        if self.n_train and folds.shape[0] != self.n_train:
            raise ValueError("folds must have one id per train row")
        if n_folds is None:
            n_folds = int(folds.max()) + 1 if folds.size else 1
        _check(lib().knn_group_set_folds(self._h, _ptr(folds), int(n_folds)))

    def kfold_sweep(self, ks, metric=L2, confusion=False, labels=True):
        """Classifier.kfold_sweep over the group (mode 0; mode 1 raises
        KnnError): rank r sweeps folds r, r + G, ...; returns as lgo_sweep."""
        ks = np.ascontiguousarray(ks, dtype=np.int32).reshape(-1)
        nk, n = ks.shape[0], self.n_train
        if not labels and not confusion:
            raise ValueError("labels=False needs confusion=True")
        C = self.class_cnt
        out_lab = np.empty((nk, n), np.int32) if labels else None
        correct = np.zeros(nk, np.int64)
        conf = np.zeros((nk, C, C), np.int64) if confusion else None
        unl = np.zeros(nk, np.int64) if confusion else None
        _check(lib().knn_group_kfold_sweep(self._h, _ptr(ks), nk, int(metric), _ptr(out_lab),
                                           _ptr(correct), _ptr(conf), _ptr(unl)))
        out = (out_lab, correct) if labels else (correct,)
        if confusion:
            out += (conf, unl)
        return out

    def last_compute_seconds(self):
        return float(lib().knn_group_last_compute_seconds(self._h))

    def normalize(self, *sets):
        """Sharded normalisation of host sets in place with an RCCL MAX/MIN
        all-reduce of the bounds (cpp:229-306)."""
        ptrs, rows, ns, d = _set_arrays(sets)
        _check(lib().knn_group_normalize(self._h, ptrs, rows, ns, d))


def run_driver(cfg: KnnConfig, workdir, gpus=1, mode="query", extra=()):
    """Runs the native drop-in driver (bin/knn_mpi_amd) the way `mpiexec
    knn_mpi` runs the reference, in `workdir`; returns its stdout.
    `extra` takes further driver flags, e.g. ["--K_list", "1,3,5"] (needs
    Validation: one search scores every K on the validation set, prints
    "K = <k> accuracy = <acc>" per K and "selected K = <k>", and the test
    pass runs at the selected K), or ["--loo", "--K_list", "1,3,5"] (no
    validation file: every K is scored by leave-one-out on the train set,
    "K = <k> loo accuracy = <acc>" per K), or ["--weights", "distance"]
    (every pass votes with weight 1 / distance, Classifier.set_vote; the
    outputs keep their format)."""
    if not os.path.exists(DRIVER_PATH):
        raise KnnError("driver not built: " + DRIVER_PATH)
    args = [DRIVER_PATH]
    for f in ("dim", "K", "N_train", "N_test", "N_val", "class_cnt"):
        args += ["--" + f, str(getattr(cfg, f))]
    for f in ("Euclidean_distance", "Normalize", "Validation"):
        args += ["--" + f, "true" if getattr(cfg, f) else "false"]
    args += ["--train_file", cfg.train_file_name, "--validation_file", cfg.validation_file_name,
             "--test_file", cfg.test_file_name, "--gpus", str(gpus), "--mode", mode]
    args += list(extra)
    r = subprocess.run(args, cwd=workdir, capture_output=True, text=True)
    if r.returncode != 0:
        raise KnnError("driver failed (%d): %s" % (r.returncode, r.stderr.strip()))
    return r.stdout
