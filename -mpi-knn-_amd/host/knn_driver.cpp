// knn_driver.cpp -- drop-in replacement for the reference program
// (/root/reference/knn_mpi.cpp main(), cpp:86-399) on MI355X GPUs.
//
// Same inputs, same outputs:
//   * config: the reference's constants (cpp:108-119) become flags with the
//     same names and defaults: --dim 784 --K 50 --N_train 60000
//     --N_test 10000 --N_val 10000 --class_cnt 10 --Euclidean_distance true
//     --Normalize true --Validation true --train_file mnist_train.csv
//     --validation_file mnist_validation.csv --test_file mnist_test.csv
//   * inputs: the same CSV formats (cpp:154-222, see csv.h)
//   * outputs: "accuracy = <cout default>" (cpp:348), Test_label.csv one
//     label per line (cpp:390-392), "Running time is <t> second" (cpp:398)
// Extra flags: --gpus N (default 1), --mode query|train (multi-GPU layout),
// --strict (exit 1 unless N_* divisible by --gpus, as MPI_Abort cpp:127-129),
// --threads T (CSV parsing threads), --output path, --timings (per-phase
// seconds on stderr; stdout stays the reference's), --tune KEY=VALUE (a
// tuning key of the library, knn_set_tuning; repeatable -- e.g. --tune i8l1=1
// for the Manhattan pass on int8 codes of byte-valued CSVs, --tune u16l1=1
// for the one on 16-bit fixed-point codes of any data, normalised included,
// --tune u16l1w=1 for the same at 256 < dim <= 1024),
// --K_list k1,k2,... (needs --Validation true): the validation pass scores
// every K of the list from one search (knn_group_classify_sweep), prints
// "K = <k> accuracy = <acc>" per K in list order, selects the first K whose
// accuracy strictly exceeds the running best (the reference's first-to-exceed
// idiom, cpp:332-335), prints "selected K = <k>" and the reference's
// "accuracy = <acc>" line for it, and runs the test pass at that K.
// --loo (needs --K_list; no validation file is read): the validation pass is
// replaced by a leave-one-out sweep of the train set (knn_group_loo_sweep:
// every train row classified against all the others), prints "K = <k> loo
// accuracy = <acc>" per K, selects K the same way and runs the test pass.
// --groups FILE (needs --loo --K_list): FILE holds one integer group id >= 0
// per train row (read like the other CSV files, one value per row); the sweep
// becomes leave-one-GROUP-out (knn_group_lgo_sweep: every train row judged
// against the rows of all the other groups -- samples of one subject, copies
// of one image), prints "K = <k> lgo accuracy = <acc>" per K and selects K the
// same way.  Without the flag stdout is unchanged.
// --kfold F (needs --K_list, 2 <= F <= 64, not with --loo; no validation file
// is read): F-fold cross-validation on fold shards (knn_group_set_folds,
// knn_group_kfold_sweep: every train row judged against the rows of the other
// folds), prints "K = <k> kfold accuracy = <acc>" per K and selects K the same
// way.  --folds FILE holds one fold id in [0, F) per train row (read like
// --groups); without it row r is in fold r % F.
// --confusion (with the default validation pass, --K_list or --loo): after that
// pass's lines prints "confusion K = <k>" for the selected K, then class_cnt
// lines of class_cnt space-separated counts (row = true class, column =
// predicted class) and "unlabelled = <n>" (queries whose label or truth is
// outside [0, class_cnt)), from knn_group_classify_sweep_eval /
// knn_group_loo_sweep_eval; without the flag stdout is unchanged.
// --weights uniform|distance (default uniform): how the neighbours vote
// (knn_group_set_vote).  distance = each neighbour weighs 1 / its distance and
// exact matches alone decide (KNN_VOTE_DISTANCE, knn_amd.h); it applies to the
// validation pass, the test pass, --K_list, --loo and --confusion, and every
// output keeps its format.
// --csv host|gpu (default host): who parses the three CSV files.  host is the
// multi-threaded reader of csv.cpp; gpu reads them through knn_csv_read on a
// context of device 0 (the text is uploaded and converted by a kernel, the few
// tokens it cannot certify by atof / atoi on the host): the same values bit
// for bit, so stdout and Test_label.csv do not change.  With --timings the
// "csv" line is followed by its parts (read, h2d, parse, d2h, slow) and the
// number of slow tokens.
// The timed region spans the same work as the reference (barrier to
// barrier: CSV parsing, distribution, normalisation, both passes, output).
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "csv.h"
#include "knn_amd.h"

namespace {

struct Config {
  int dim = 784;
  int K = 50;
  long long N_train = 60000, N_test = 10000, N_val = 10000;
  int class_cnt = 10;
  bool Euclidean_distance = true, Normalize = true, Validation = true;
  std::string train_file = "mnist_train.csv";
  std::string validation_file = "mnist_validation.csv";
  std::string test_file = "mnist_test.csv";
  std::string output = "Test_label.csv";
  int gpus = 1;
  int mode = 0;
  bool strict = false;
  int threads = 0;
  bool timings = false;
  std::vector<int32_t> K_list;  // --K_list (empty: the single --K)
  bool loo = false;             // --loo: judge the K of --K_list by leave-one-out on the train set
  std::string groups_file;      // --groups: with --loo, leave out the row's whole group
  int kfold = 0;                // --kfold F: judge the K of --K_list by F-fold cross-validation
  std::string folds_file;       // --folds: one fold id per train row (default: row % F)
  bool confusion = false;       // --confusion: print the selected K's confusion matrix
  int vote = KNN_VOTE_UNIFORM;  // --weights uniform|distance
  bool csv_gpu = false;         // --csv gpu: the files are parsed on device 0
  std::vector<std::pair<std::string, long long>> tune;  // --tune KEY=VALUE (knn_set_tuning keys)
};

bool parse_bool(const std::string& v) { return v == "true" || v == "1" || v == "yes"; }

void usage() {
  fprintf(stderr,
          "usage: knn_mpi_amd [--dim D] [--K K] [--N_train N] [--N_test N] [--N_val N]\n"
          "  [--class_cnt C] [--Euclidean_distance true|false] [--Normalize true|false]\n"
          "  [--Validation true|false] [--train_file F] [--validation_file F]\n"
          "  [--test_file F] [--output F] [--gpus G] [--mode query|train] [--strict]\n"
          "  [--threads T] [--timings] [--K_list K1,K2,...] [--loo] [--confusion]\n"
          "  [--groups F] [--kfold F] [--folds FILE]\n"
          "  [--tune KEY=VALUE]... [--weights uniform|distance] [--csv host|gpu]\n"
          "  --K_list needs --Validation true: one search scores every K on the validation\n"
          "  set; the test pass runs at the first K with the best accuracy\n"
          "  --loo needs --K_list: scores every K by leave-one-out on the train set instead\n"
          "  (no validation file is read)\n"
          "  --groups F needs --loo --K_list: F holds one integer group id per train row;\n"
          "  every row is judged without the rows of its own group (leave-one-group-out)\n"
          "  --kfold F needs --K_list: scores every K by F-fold cross-validation on the train\n"
          "  set (2 <= F <= 64; every row judged without the rows of its own fold; no\n"
          "  validation file is read; not together with --loo); --folds FILE holds one fold\n"
          "  id in [0, F) per train row, without it row r is in fold r mod F\n"
          "  --confusion prints the confusion matrix of the validation (or --loo) pass at the\n"
          "  selected K: class_cnt rows (true class) of class_cnt counts (predicted class)\n"
          "  --weights distance: every pass votes with weight 1 / distance (exact matches\n"
          "  alone decide where there are any); uniform (default) is the reference's vote\n"
          "  --tune sets a tuning key of the library (knn_amd.h, knn_set_tuning), e.g.\n"
          "  --tune i8l1=1: the L1 pass on int8 codes for byte-coded data at dim <= 256\n"
          "  (i8l1=2: also at 256 < dim <= 1024); --tune u16l1=1: the L1 pass on 16-bit\n"
          "  fixed-point codes for any data at dim <= 256 (--Normalize true included);\n"
          "  --tune u16l1w=1: the same at 256 < dim <= 1024 (the default dim = 784)\n"
          "  --csv gpu parses the CSV files on GPU 0 (same values as the default host reader)\n");
}

// "1,3,5" -> {1, 3, 5}; false on an empty list, an empty item or a non-digit
bool parse_k_list(const std::string& v, std::vector<int32_t>& out) {
  out.clear();
  size_t i = 0;
  while (true) {
    long long k = 0;
    size_t digits = 0;
    for (; i < v.size() && v[i] >= '0' && v[i] <= '9'; ++i, ++digits) {
      k = k * 10 + (v[i] - '0');
      if (k > INT32_MAX) return false;
    }
    if (!digits) return false;
    out.push_back((int32_t)k);
    if (i == v.size()) return true;
    if (v[i++] != ',') return false;
  }
}

int parse_args(int argc, char** argv, Config& c) {
  for (int i = 1; i < argc; i++) {
    std::string a = argv[i];
    if (a == "-h" || a == "--help") { usage(); exit(0); }
    if (a.rfind("--", 0) != 0) { usage(); return 1; }
    a = a.substr(2);
    std::string v;
    size_t eq = a.find('=');
    if (eq != std::string::npos) { v = a.substr(eq + 1); a = a.substr(0, eq); }
    else if (a == "strict") { c.strict = true; continue; }
    else if (a == "timings") { c.timings = true; continue; }
    else if (a == "loo") { c.loo = true; continue; }
    else if (a == "confusion") { c.confusion = true; continue; }
    else if (i + 1 < argc) v = argv[++i];
    else { usage(); return 1; }
    if (a == "dim") c.dim = atoi(v.c_str());
    else if (a == "K") c.K = atoi(v.c_str());
    else if (a == "N_train") c.N_train = atoll(v.c_str());
    else if (a == "N_test") c.N_test = atoll(v.c_str());
    else if (a == "N_val") c.N_val = atoll(v.c_str());
    else if (a == "class_cnt") c.class_cnt = atoi(v.c_str());
    else if (a == "Euclidean_distance") c.Euclidean_distance = parse_bool(v);
    else if (a == "Normalize") c.Normalize = parse_bool(v);
    else if (a == "Validation") c.Validation = parse_bool(v);
    else if (a == "train_file") c.train_file = v;
    else if (a == "validation_file") c.validation_file = v;
    else if (a == "test_file") c.test_file = v;
    else if (a == "output") c.output = v;
    else if (a == "groups") c.groups_file = v;
    else if (a == "kfold") c.kfold = atoi(v.c_str());
    else if (a == "folds") c.folds_file = v;
    else if (a == "gpus") c.gpus = atoi(v.c_str());
    else if (a == "mode") c.mode = (v == "train" || v == "1") ? 1 : 0;
    else if (a == "strict") c.strict = parse_bool(v);
    else if (a == "threads") c.threads = atoi(v.c_str());
    else if (a == "loo") c.loo = parse_bool(v);
    else if (a == "confusion") c.confusion = parse_bool(v);
    else if (a == "K_list") {
      if (!parse_k_list(v, c.K_list)) {
        fprintf(stderr, "--K_list takes a comma-separated list of non-negative integers\n");
        return 1;
      }
    }
    else if (a == "weights") {
      if (v == "uniform") c.vote = KNN_VOTE_UNIFORM;
      else if (v == "distance") c.vote = KNN_VOTE_DISTANCE;
      else {
        fprintf(stderr, "--weights takes uniform or distance\n");
        return 1;
      }
    }
    else if (a == "csv") {
      if (v == "host") c.csv_gpu = false;
      else if (v == "gpu") c.csv_gpu = true;
      else {
        fprintf(stderr, "--csv takes host or gpu\n");
        return 1;
      }
    }
    else if (a == "tune") {
      const size_t e = v.find('=');
      char* end = nullptr;
      const long long val = e == std::string::npos ? 0 : strtoll(v.c_str() + e + 1, &end, 10);
      if (e == std::string::npos || e == 0 || end == v.c_str() + e + 1 || *end) {
        fprintf(stderr, "--tune takes KEY=VALUE with an integer value\n");
        return 1;
      }
      c.tune.emplace_back(v.substr(0, e), val);
    }
    else { fprintf(stderr, "unknown flag --%s\n", a.c_str()); usage(); return 1; }
  }
  return 0;
}

[[noreturn]] void die(const std::string& msg) {
  fprintf(stderr, "knn_mpi_amd: %s\n", msg.c_str());
  exit(1);  // ≙ MPI_Abort(MPI_COMM_WORLD, 1)
}

// --csv gpu: the context the files are parsed on, the sums of their parts
struct GpuCsv {
  knn_ctx* ctx = nullptr;
  double parts[5] = {0, 0, 0, 0, 0};  // read, h2d, parse, d2h, slow
  int64_t slow = 0;
};

void load(const std::string& path, int dim, bool with_label, int64_t rows, std::vector<double>& X,
          std::vector<int32_t>* lab, int threads, GpuCsv* gpu) {
  X.assign((size_t)rows * dim, 0.0);
  if (lab) lab->assign((size_t)rows, 0);
  int64_t tokens = 0;
  if (gpu) {
    if (knn_csv_read(gpu->ctx, path.c_str(), dim, with_label, rows, X.data(),
                     lab ? lab->data() : nullptr, &tokens))
      die(knn_last_error());
    double parts[5];
    if (knn_csv_last_phases(gpu->ctx, parts)) die(knn_last_error());
    for (int i = 0; i < 5; i++) gpu->parts[i] += parts[i];
    gpu->slow += knn_csv_last_slow(gpu->ctx);
  } else {
    knnhost::CsvResult r = knnhost::read_csv(path, dim, with_label, rows, X.data(),
                                             lab ? lab->data() : nullptr, threads);
    if (!r.ok) die(r.error);
    tokens = r.tokens;
  }
  const int64_t want = rows * (dim + (with_label ? 1 : 0));
  if (tokens != want)
    die(path + ": expected " + std::to_string(want) + " values, found " + std::to_string(tokens));
}

// "confusion K = <k>", the C x C matrix of list entry `sel` (conf: [nk][C][C]),
// "unlabelled = <n>"
void print_confusion(int32_t k, int C, const int64_t* conf, int64_t unl) {
  std::cout << "confusion K = " << k << std::endl;
  for (int t = 0; t < C; t++) {
    for (int p = 0; p < C; p++) std::cout << (p ? " " : "") << conf[(size_t)t * C + p];
    std::cout << std::endl;
  }
  std::cout << "unlabelled = " << unl << std::endl;
}

}  // namespace

int main(int argc, char** argv) {
  Config c;
  if (parse_args(argc, argv, c)) return 1;
  if (c.threads <= 0) c.threads = (int)std::max(1u, std::thread::hardware_concurrency());
  if (c.threads > 16) c.threads = 16;
  if (c.gpus < 1) die("--gpus must be >= 1");
  if (c.dim <= 0 || c.K < 0 || c.N_train <= 0 || c.N_test < 0 || c.N_val < 0 || c.class_cnt <= 0)
    die("bad configuration");
  if (c.loo && c.K_list.empty()) die("--loo needs --K_list (the K to judge by leave-one-out)");
  if (!c.groups_file.empty() && (!c.loo || c.K_list.empty()))
    die("--groups needs --loo --K_list (the groups are left out of the leave-one-out sweep)");
  if (c.kfold && c.loo) die("--kfold and --loo exclude each other (one way to judge K)");
  if (c.kfold && (c.kfold < 2 || c.kfold > 64)) die("--kfold takes a fold count in [2, 64]");
  if (c.kfold && c.K_list.empty()) die("--kfold needs --K_list (the K to judge by cross-validation)");
  if (!c.folds_file.empty() && !c.kfold) die("--folds needs --kfold F --K_list");
  if (c.loo || c.kfold) c.Validation = false;  // the train set is its own validation set: no file is read
  if (c.strict && (c.N_train % c.gpus || c.N_test % c.gpus || (c.Validation && c.N_val % c.gpus)))
    die("N_train/N_test/N_val not divisible by the number of GPUs (--strict, cpp:127-129)");
  if (!c.K_list.empty()) {
    if (!c.loo && !c.kfold && !c.Validation)
      die("--K_list needs --Validation true (K is judged on the validation set)");
    if (!c.loo && !c.kfold && c.N_val <= 0) die("--K_list needs a validation set (N_val > 0)");
    if (c.K_list.size() > 4096) die("--K_list takes at most 4096 values");
    for (size_t i = 0; i < c.K_list.size(); i++) {
      if (c.K_list[i] > c.N_train)
        die("--K_list entry " + std::to_string(c.K_list[i]) + " exceeds N_train");
      if (c.loo && c.K_list[i] > c.N_train - 1)
        die("--K_list entry " + std::to_string(c.K_list[i]) +
            " exceeds N_train - 1 (--loo takes the row itself out)");
    }
  }

  knn_group* g = nullptr;
  if (knn_group_create(&g, c.gpus, nullptr, c.mode)) die(knn_last_error());
  for (const auto& kv : c.tune)
    if (knn_group_set_tuning(g, kv.first.c_str(), kv.second)) die(knn_last_error());
  if (knn_group_set_vote(g, c.vote)) die(knn_last_error());
  GpuCsv gpu_csv;
  if (c.csv_gpu && knn_create(&gpu_csv.ctx, 0)) die(knn_last_error());
  GpuCsv* gc = c.csv_gpu ? &gpu_csv : nullptr;

  using clk = std::chrono::steady_clock;
  const auto start = clk::now();  // ≙ MPI_Barrier + MPI_Wtime, cpp:133-134
  auto mark = start;
  auto phase = [&](const char* name) {
    const auto now = clk::now();
    if (c.timings)
      fprintf(stderr, "[knn_mpi_amd] %-10s %.3f s\n", name,
              std::chrono::duration<double>(now - mark).count());
    mark = now;
  };

  std::vector<double> Xtr, Xte, Xva;
  std::vector<int32_t> Ltr, Lva;
  load(c.train_file, c.dim, true, c.N_train, Xtr, &Ltr, c.threads, gc);
  load(c.test_file, c.dim, false, c.N_test, Xte, nullptr, c.threads, gc);
  if (c.Validation) load(c.validation_file, c.dim, true, c.N_val, Xva, &Lva, c.threads, gc);
  std::vector<int32_t> groups;  // --groups: one id per train row
  int32_t n_groups = 0;
  if (!c.groups_file.empty()) {
    std::vector<double> Gv;
    load(c.groups_file, 1, false, c.N_train, Gv, nullptr, c.threads, gc);
    groups.resize((size_t)c.N_train);
    for (long long i = 0; i < c.N_train; i++) {
      const double v = Gv[(size_t)i];
      if (!(v >= 0.0 && v < (double)INT32_MAX) || v != (double)(int32_t)v)
        die(c.groups_file + ": row " + std::to_string(i) + " is not an integer group id >= 0");
      groups[(size_t)i] = (int32_t)v;
      n_groups = std::max(n_groups, groups[(size_t)i] + 1);
    }
  }
  std::vector<int32_t> folds;  // --kfold: one fold id per train row
  if (c.kfold) {
    folds.resize((size_t)c.N_train);
    if (c.folds_file.empty()) {
      for (long long i = 0; i < c.N_train; i++) folds[(size_t)i] = (int32_t)(i % c.kfold);
    } else {
      std::vector<double> Fv;
      load(c.folds_file, 1, false, c.N_train, Fv, nullptr, c.threads, gc);
      for (long long i = 0; i < c.N_train; i++) {
        const double v = Fv[(size_t)i];
        if (!(v >= 0.0 && v < (double)c.kfold) || v != (double)(int32_t)v)
          die(c.folds_file + ": row " + std::to_string(i) + " is not an integer fold id in [0, F)");
        folds[(size_t)i] = (int32_t)v;
      }
    }
  }
  phase("csv");
  if (gc && c.timings) {
    static const char* const names[5] = {"read", "h2d", "parse", "d2h", "slow"};
    for (int i = 0; i < 5; i++)
      fprintf(stderr, "[knn_mpi_amd]   csv.%-6s %.3f s\n", names[i], gc->parts[i]);
    fprintf(stderr, "[knn_mpi_amd]   csv slow tokens %lld\n", (long long)gc->slow);
  }
  if (gc) mark = clk::now();  // (the lines above are not part of the next phase)

  if (c.Normalize) {  // cpp:229-306 on the GPUs: sharded min/max + RCCL all-reduce + apply
    std::vector<double*> sets{Xtr.data(), Xte.data()};
    std::vector<int64_t> rows{c.N_train, c.N_test};
    if (c.Validation) { sets.push_back(Xva.data()); rows.push_back(c.N_val); }
    if (knn_group_normalize(g, sets.data(), rows.data(), (int32_t)sets.size(), c.dim))
      die(knn_last_error());
  }
  phase("normalize");

  if (knn_group_set_train(g, Xtr.data(), Ltr.data(), c.N_train, c.dim, c.class_cnt))
    die(knn_last_error());
  phase("set_train");
  const int metric = c.Euclidean_distance ? KNN_METRIC_L2 : KNN_METRIC_L1;
  const size_t cc = (size_t)c.class_cnt * c.class_cnt;

  if (c.kfold) {  // cpp:308-349 with every train row judged against the other folds' rows
    const int32_t nk = (int32_t)c.K_list.size();
    std::vector<int32_t> pred((size_t)nk * c.N_train);
    std::vector<int64_t> correct(nk, 0);
    std::vector<int64_t> conf(c.confusion ? nk * cc : 0, 0), unl(c.confusion ? nk : 0, 0);
    if (knn_group_set_folds(g, folds.data(), c.kfold)) die(knn_last_error());
    if (knn_group_kfold_sweep(g, c.K_list.data(), nk, metric, pred.data(), correct.data(),
                              c.confusion ? conf.data() : nullptr,
                              c.confusion ? unl.data() : nullptr))
      die(knn_last_error());
    double best = -1.0;
    int32_t sel = 0;
    for (int32_t i = 0; i < nk; i++) {
      double acc = (double)correct[i];  // acc_calc, cpp:69-84
      acc /= c.N_train;
      std::cout << "K = " << c.K_list[i] << " kfold accuracy = " << acc << std::endl;
      if (acc > best) {  // first to strictly exceed, like cpp:332-335
        best = acc;
        c.K = c.K_list[i];
        sel = i;
      }
    }
    std::cout << "selected K = " << c.K << std::endl;
    if (c.confusion) print_confusion(c.K, c.class_cnt, conf.data() + sel * cc, unl[sel]);
    phase("kfold");
  } else if (c.loo) {  // cpp:308-349 with every train row judged against all the others
    const int32_t nk = (int32_t)c.K_list.size();
    std::vector<int32_t> pred((size_t)nk * c.N_train);
    std::vector<int64_t> correct(nk, 0);
    std::vector<int64_t> conf(c.confusion ? nk * cc : 0, 0), unl(c.confusion ? nk : 0, 0);
    const bool lgo = !groups.empty();
    if (lgo) {  // every row without the rows of its own group
      if (knn_group_set_groups(g, groups.data(), n_groups)) die(knn_last_error());
      if (knn_group_lgo_sweep(g, c.K_list.data(), nk, metric, pred.data(), correct.data(),
                              c.confusion ? conf.data() : nullptr,
                              c.confusion ? unl.data() : nullptr))
        die(knn_last_error());
    } else if (c.confusion
                   ? knn_group_loo_sweep_eval(g, c.K_list.data(), nk, metric, pred.data(),
                                              correct.data(), conf.data(), unl.data())
                   : knn_group_loo_sweep(g, c.K_list.data(), nk, metric, pred.data(),
                                         correct.data()))
      die(knn_last_error());
    double best = -1.0;
    int32_t sel = 0;
    for (int32_t i = 0; i < nk; i++) {
      double acc = (double)correct[i];  // acc_calc, cpp:69-84
      acc /= c.N_train;
      std::cout << "K = " << c.K_list[i] << (lgo ? " lgo" : " loo") << " accuracy = " << acc
                << std::endl;
      if (acc > best) {  // first to strictly exceed, like cpp:332-335
        best = acc;
        c.K = c.K_list[i];
        sel = i;
      }
    }
    std::cout << "selected K = " << c.K << std::endl;
    if (c.confusion) print_confusion(c.K, c.class_cnt, conf.data() + sel * cc, unl[sel]);
    phase("loo");
  } else if (!c.K_list.empty()) {  // the validation pass (cpp:308-349) for every K of the list
    const int32_t nk = (int32_t)c.K_list.size();
    std::vector<int32_t> pred((size_t)nk * c.N_val);
    std::vector<int64_t> correct(nk, 0);
    std::vector<int64_t> conf(c.confusion ? nk * cc : 0, 0), unl(c.confusion ? nk : 0, 0);
    if (c.confusion
            ? knn_group_classify_sweep_eval(g, Xva.data(), c.N_val, c.K_list.data(), nk, metric,
                                            pred.data(), Lva.data(), correct.data(), conf.data(),
                                            unl.data())
            : knn_group_classify_sweep(g, Xva.data(), c.N_val, c.K_list.data(), nk, metric,
                                       pred.data(), Lva.data(), correct.data()))
      die(knn_last_error());
    double best = -1.0, best_acc = 0.0;
    int32_t sel = 0;
    for (int32_t i = 0; i < nk; i++) {
      double acc = (double)correct[i];  // acc_calc, cpp:69-84
      acc /= c.N_val;
      std::cout << "K = " << c.K_list[i] << " accuracy = " << acc << std::endl;
      if (acc > best) {  // first to strictly exceed, like cpp:332-335
        best = acc;
        best_acc = acc;
        c.K = c.K_list[i];
        sel = i;
      }
    }
    std::cout << "selected K = " << c.K << std::endl;
    std::cout << "accuracy = " << best_acc << std::endl;
    if (c.confusion) print_confusion(c.K, c.class_cnt, conf.data() + sel * cc, unl[sel]);
    phase("validation");
  } else if (c.Validation) {  // cpp:308-349
    std::vector<int32_t> pred(c.N_val);
    if (c.N_val > 0 &&
        knn_group_classify(g, Xva.data(), c.N_val, c.K, metric, pred.data(), nullptr, nullptr, nullptr))
      die(knn_last_error());
    double acc = 0;  // acc_calc, cpp:69-84
    for (long long i = 0; i < c.N_val; i++)
      if (Lva[i] == pred[i]) acc++;
    acc /= c.N_val;
    std::cout << "accuracy = " << acc << std::endl;
    if (c.confusion && c.N_val > 0) {  // the same pass as a one-K sweep, for its matrix
      const int32_t k1 = c.K;
      std::vector<int64_t> conf(cc, 0);
      int64_t unl = 0;
      if (knn_group_classify_sweep_eval(g, Xva.data(), c.N_val, &k1, 1, metric, nullptr, Lva.data(),
                                        nullptr, conf.data(), &unl))
        die(knn_last_error());
      print_confusion(c.K, c.class_cnt, conf.data(), unl);
    }
    phase("validation");
  }

  std::vector<int32_t> test_lab(c.N_test);  // cpp:352-393
  if (c.N_test > 0 &&
      knn_group_classify(g, Xte.data(), c.N_test, c.K, metric, test_lab.data(), nullptr, nullptr, nullptr))
    die(knn_last_error());
  phase("test");
  {
    // one label per line (cpp:390-392; '\n' without a flush per line)
    std::ofstream outfile(c.output);
    for (long long i = 0; i < c.N_test; i++) outfile << test_lab[i] << '\n';
  }
  phase("output");

  const auto finish = clk::now();  // cpp:395-396
  knn_group_destroy(g);
  if (gpu_csv.ctx) knn_destroy(gpu_csv.ctx);
  std::cout << "Running time is " << std::chrono::duration<double>(finish - start).count()
            << " second" << std::endl;
  return 0;
}
