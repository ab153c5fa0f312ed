// plan_check.cpp -- walks plan_search (csrc/knn_plan.cpp) over a grid of
// shapes, precisions and tuning values on a CPU and checks, for every plan
// that names a kernel, what the launch code of knn_run_search relies on:
// buffer sizes, grid sizes and the template instance all follow from the
// plan.  Links knn_plan.cpp only (no HIP, no library); the kernels' facts
// are faked over the values builds have had.  Prints one line per violation
// and exits non-zero if there was one.
//
//   make -C -mpi-knn-_amd bin/plan_check && -mpi-knn-_amd/bin/plan_check
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <vector>

#include "../include/knn_amd.h"
#include "knn_plan.h"

using namespace knnk;

namespace {

// the fake kernels' properties for the current pass over the grid
int g_blocks = 2, g_qpw5 = 32, g_trows = 128;

int fake_blocks(int, int, int, int) { return g_blocks; }
int fake_s3q_blocks() { return 1; }
int fake_qpw(int metric, int) { return metric == 5 ? g_qpw5 : 32; }
int fake_trows(int metric, int DP) {
  if ((metric == 2 || metric == 4) && DP > 256) return kS3Rows;
  // (knn_cand_sad.hip's own tiles; knn_cand_sad_wide.hip's above 256 dims)
  if (metric == 7) return DP > 128 ? 64 : 128;
  return DP <= 256 ? g_trows : 128;
}
// (no build has had a query-resident kernel beyond 30 chunks, DP = 960)
bool fake_qres(int DP) { return DP % 64 == 0 && DP <= 960; }
const KernelFacts kFake = {fake_blocks, fake_s3q_blocks, fake_qpw, fake_trows, fake_qres};

long g_plans = 0, g_named = 0, g_bad = 0;

struct Shape {
  int d;
  int64_t n, m;
  int W, metric, precision;
  bool i8_ok;
};

void fail(const Shape& sh, const char* tkey, int64_t tval, const SearchPlan& p, const char* what) {
  if (++g_bad > 200) return;  // (enough to read)
  printf("VIOLATION %s: d=%d n=%lld m=%lld W=%d metric=%d precision=%d i8_ok=%d tune %s=%lld "
         "facts(blocks=%d qpw5=%d trows=%d) -> %s S=%d R=%d lps=%d NL=%d C=%d n_qt=%d qpb=%d "
         "m_pad=%lld n_tiles=%lld G=%d gk=%d active=%d\n",
         what, sh.d, (long long)sh.n, (long long)sh.m, sh.W, sh.metric, sh.precision, sh.i8_ok,
         tkey, (long long)tval, g_blocks, g_qpw5, g_trows, p.kernel, p.S, p.R, p.lps, p.NL, p.C,
         p.n_qt, p.qpb, (long long)p.m_pad, (long long)p.n_tiles, p.G, p.gk, p.active);
}

// the list lengths each kernel family is instantiated for
bool list_len_instantiated(const SearchPlan& p) {
  const int R = p.R;
  if (p.qres || p.s3q) return R == 8;
  if (p.s3 || (p.DP > 256 && p.kmetric != 7)) return R == 8 || R == 16;
  switch (p.kmetric) {
    case 1: return R == 8 || R == 16;
    case 3: case 4: return R == 4;
    case 5: case 6: return R == 4 || R == 8;
    case 7: return R == 8 || R == 16;
    default: return R == 4 || R == 8 || R == 16;
  }
}

void check(const Shape& sh, const Tuning& tune, const char* tkey, int64_t tval) {
  const int64_t n_pad = (sh.n + 255) / 256 * 256;
  const PlanIn in{sh.n, n_pad, sh.d, pad_dim(sh.d), sh.metric, sh.m, sh.W, sh.precision,
                  false, false, sh.i8_ok, region_count(tune, sh.i8_ok, sh.n, sh.d),
                  norm_blocks_on(tune, sh.i8_ok, sh.n, sh.d), 256, (g_plans & 1) != 0, tune, kFake};
  const SearchPlan p = plan_search(in);
  ++g_plans;
  if (!p.ok) return;  // "no kernel" is a value: the search refuses before it allocates
  ++g_named;
#define REQUIRE(cond) do { if (!(cond)) fail(sh, tkey, tval, p, #cond); } while (0)
  REQUIRE(p.kernel[0] != 0);
  REQUIRE(p.S >= 1 && p.S <= std::min<int64_t>(64, p.n_tiles));
  REQUIRE(p.lps == 2 || p.lps == 4);
  REQUIRE(p.NL == p.lps * p.S);
  REQUIRE(p.C >= 1 && p.C <= p.NL * p.R && p.C <= kMaxUnion);
  REQUIRE(p.m_pad == (int64_t)p.n_qt * p.qpb && p.m_pad >= sh.m && p.m_pad - sh.m < p.qpb);
  if (!p.s3 && (p.DP <= 256 || p.kmetric == 7)) REQUIRE(p.qpb == p.qpw * p.nw);
  REQUIRE(p.gk >= 0 && p.gk <= (p.s3 ? 16 : 4));
  REQUIRE(p.G == 4 || p.G == 8);
  REQUIRE(p.gmask == (p.gk ? p.G - 1 : 3));
  REQUIRE(p.active >= 1 && p.active <= p.S && p.active <= kGthrSlots);
  REQUIRE(list_len_instantiated(p));
  REQUIRE(!p.qres || p.s3q);
  REQUIRE(!p.s3q || p.s3h);
  REQUIRE(!p.use_gthr || (!p.s3 && (p.DP <= 256 || p.kmetric == 7)) || p.s3q);
  REQUIRE(!p.gthr_init || p.use_gthr);
  REQUIRE(p.n_tiles >= 1 && p.n_tiles * p.trows == (p.s3 ? p.n_pad3 : n_pad));
  REQUIRE(p.qblk >= 0 && p.qblk <= p.n_qt);
  REQUIRE(!p.i8resc || p.kmetric == 6);
  REQUIRE(!p.query_order || (in.ord_P > 0 && p.kmetric >= 4 && !p.s3));
  REQUIRE(p.cap >= 1 && p.cap <= sh.m);
  // path 7 (L1 on int8 codes): only for L1 on an integer-coded set and never
  // with the key at 0; "i8" alone does not reach it.  At d <= 256: the key at
  // 1 or 2, or AUTO's rule; the plain int8 image at pad_dim_i8w.  At 256 < d
  // <= 1024: the key at 2 only (never AUTO's choice, so it arms no AUTO
  // decision); plain rows at pad_dim_i8l1w, the wide kernel, its own query
  // tile and tile rows.  Either way the fp32 L1 kernel's list layout, one
  // list per lane, R 8 or 16, no query order, no int8 rescan filter.
  if (p.kmetric == 7) {
    REQUIRE(sh.metric == KNN_METRIC_L1 && sh.i8_ok && sh.d <= 1024 && tune.i8l1 != 0);
    if (sh.d <= 256) {
      REQUIRE(tune.i8l1 >= 1 || (sh.precision == KNN_PRECISION_AUTO && sh.m >= 4096 && sh.W <= 64));
      REQUIRE(p.image == IMG_I8 && p.DP == pad_dim_i8w(sh.d));
      REQUIRE(!strncmp(p.kernel, "cand_sad_kernel<", 16));
    } else {
      REQUIRE(tune.i8l1 == 2);
      REQUIRE(p.image == IMG_I8W && p.DP == pad_dim_i8l1w(sh.d) && p.DP > 256 && p.DP % 16 == 0);
      REQUIRE(p.DP >= sh.d && p.DP - sh.d < 16);
      REQUIRE(!strncmp(p.kernel, "cand_sad_wide_kernel<", 21));
      REQUIRE(p.trows == fake_trows(7, p.DP) && p.qpb == 32 * p.nw);
    }
    REQUIRE(p.i8_swz == 0 && p.xsw == 0);
    REQUIRE(p.lps == 2 && (p.nw == 4 || p.nw == 8) && p.qpw == 32 && !p.s3);
    REQUIRE(p.R == 8 || p.R == 16);
    REQUIRE(!p.i8resc && !p.query_order && p.seed_rows == 0);
    REQUIRE(err_factor(7, p.DP) == 0.0);
    REQUIRE(p.auto_arm == (tune.i8l1 < 0 && !p.abl));
  } else if (sh.metric == KNN_METRIC_L1) {
    REQUIRE(p.kmetric == 1);
    REQUIRE(tune.i8l1 < 1 || !sh.i8_ok || sh.d > 256);
    REQUIRE(tune.i8l1 != 2 || !sh.i8_ok || sh.d > 1024);
  }
  REQUIRE((pad_dim_i8l1w(sh.d) > 0) == (sh.d > 256 && sh.d <= 1024));
  // Above 1024 dims no code pass applies (the wide L1 passes hand over to the
  // fp32 L1 stream kernel whatever "i8l1" and "u16l1w" say), no int8 pass, no
  // query-resident kernel; the widths pad to the stream kernels' granules and
  // each precision names its stream kernel.
  if (sh.d > 1024) {
    const int d32 = (sh.d + 31) / 32 * 32, d16 = (sh.d + 15) / 16 * 16;
    REQUIRE(pad_dim(sh.d) == d32 && pad_dim_fp16_s3(sh.d) == d32 && pad_dim_bf16x3(sh.d) == d16);
    REQUIRE(pad_dim_i8l1w(sh.d) < 0 && pad_dim_u16l1w(sh.d) < 0 && pad_dim_fp16(sh.d) < 0);
    REQUIRE(pad_dim_i8(sh.d) < 0 && pad_dim_i8w(sh.d) < 0);
    REQUIRE(!p.qres && p.kmetric != 5 && p.kmetric != 6 && p.kmetric != 7 && p.kmetric != 8);
    REQUIRE(p.R == 8 || p.R == 16);
    char want[64];
    if (sh.metric == KNN_METRIC_L1) {
      REQUIRE(p.kmetric == 1 && p.DP == d32 && p.image == IMG_FP32);
      snprintf(want, sizeof want, "cand_stream_kernel<32,%d,1>", p.R);
    } else if (p.kmetric == 4) {
      REQUIRE(p.s3 && p.s3h && p.DP == d32 && p.image == IMG_FP16_S3 && (!p.s3q || p.R == 8));
      snprintf(want, sizeof want, "cand_s3_kernel<%d,true,%s>", p.R, p.s3q ? "true" : "false");
    } else if (p.kmetric == 2) {
      REQUIRE(p.s3 && !p.s3h && p.DP == d16 && p.image == IMG_BF16X3);
      snprintf(want, sizeof want, "cand_s3_kernel<%d,false,false>", p.R);
    } else {
      REQUIRE(p.kmetric == 0 && p.DP == d32 && p.image == IMG_FP32);
      snprintf(want, sizeof want, "cand_stream_kernel<32,%d,0>", p.R);
    }
    REQUIRE(!strcmp(p.kernel, want));
    // the fast rescan's wide filter fits a gfx950 CU's 160 KiB at every width
    // of the grid, with at least 4 queries per pass
    const int fqw = rescan_wide_queries(pad_dim(sh.d), 160 * 1024);
    REQUIRE(fqw == (pad_dim(sh.d) <= 5088 ? 8 : 4));
    REQUIRE((int64_t)fqw * (pad_dim(sh.d) + 1) * 4 + 8 * fqw + 8 <= 160 * 1024);
  }
#undef REQUIRE
}

void walk(const Tuning& tune, const char* tkey, int64_t tval) {
  static const int ds[] = {1,    16,   24,   96,   128,  256,  257,  288,  300,  320,  784, 960,
                           1024, 1025, 1536, 2016, 2048, 3072, 4096, 4097, 5088, 5089, 6000};
  static const int64_t ns[] = {1, 255, 2000, 40000, 1000000, 12500000};
  static const int64_t ms[] = {1, 127, 4095, 4096, 10000, 131072, 1000000};
  // the path's cap: k <= 1000 on this path, W = k + 1 (and never above n)
  static const int Ws[] = {1, 2, 11, 12, 27, 28, 64, 65, 101, 102, 103, 123, 124, 1001};
  // (beyond 1025 dims nothing in the plan depends on the width but the
  // padding: a coarser walk over n and m there)
  for (int d : ds)
    for (int64_t n : ns)
      for (int64_t m : ms)
        for (int W : Ws) {
          if (d > 1025 && (n == 1 || n == 40000 || n == 12500000 || m == 4095 || m == 10000 ||
                           m == 1000000))
            continue;
          for (int metric : {KNN_METRIC_L2, KNN_METRIC_L1})
            for (int prec : {KNN_PRECISION_AUTO, KNN_PRECISION_FP32, KNN_PRECISION_BF16X3,
                             KNN_PRECISION_FP16})
              for (bool i8_ok : {false, true})
                check(Shape{d, n, m, (int)std::min<int64_t>(W, n), metric, prec, i8_ok}, tune,
                      tkey, tval);
        }
}

struct KeyValues {
  const char* key;
  int64_t def;                   // the default (walked with the default tuning)
  std::vector<int64_t> ok, bad;  // accepted edge values; values just outside
};

}  // namespace

// plan_check pads D...: one line "d pad_dim pad_dim_bf16x3 pad_dim_fp16_s3
// pad_dim_i8l1w pad_dim_u16l1w rescan_wide_queries(pad_dim, 160 KiB)" per width.
// plan_check name d n m W metric precision [key=value ...]: the kernel the
// plan names for one shape (fake facts; a continuous train set).
int cli(int argc, char** argv) {
  if (!strcmp(argv[1], "pads")) {
    for (int i = 2; i < argc; ++i) {
      const int d = atoi(argv[i]);
      printf("%d %d %d %d %d %d %d\n", d, pad_dim(d), pad_dim_bf16x3(d), pad_dim_fp16_s3(d),
             pad_dim_i8l1w(d), pad_dim_u16l1w(d), rescan_wide_queries(pad_dim(d), 160 * 1024));
    }
    return 0;
  }
  if (!strcmp(argv[1], "name") && argc >= 8) {
    const Shape sh{atoi(argv[2]), atoll(argv[3]), atoll(argv[4]), atoi(argv[5]), atoi(argv[6]),
                   atoi(argv[7]), false};
    Tuning tune;
    for (int i = 8; i < argc; ++i) {
      char* eq = strchr(argv[i], '=');
      const char* err = nullptr;
      if (!eq) return 2;
      *eq = 0;
      if (set_tuning(tune, argv[i], atoll(eq + 1), &err) != KNN_OK) return 2;
    }
    const int64_t n_pad = (sh.n + 255) / 256 * 256;
    const PlanIn in{sh.n, n_pad, sh.d, pad_dim(sh.d), sh.metric, sh.m, sh.W, sh.precision,
                    false, false, false, 0, false, 256, false, tune, kFake};
    const SearchPlan p = plan_search(in);
    printf("%s\n", p.ok ? p.kernel : "-");
    return 0;
  }
  return 2;
}

int main(int argc, char** argv) {
  if (argc > 1) return cli(argc, argv);
  // the default tuning under every fake build
  for (int blocks : {1, 2, 3, 4, 8})
    for (int qpw5 : {32, 64})
      for (int trows : {128, 256}) {
        g_blocks = blocks, g_qpw5 = qpw5, g_trows = trows;
        walk(Tuning{}, "-", 0);
      }
  // each key at each of its accepted edge values ("ablate" switches timing
  // experiments whose results are invalid: only its threshold bits here)
  const KeyValues keys[] = {
      {"fp16", -1, {-1, 0, 1}, {-2, 2}},   {"mfma16", -1, {-1, 0, 1}, {-2, 2}},
      {"R", 0, {0, 4, 8, 16}, {-1, 2, 32}}, {"nw", 0, {0, 4, 8, 16}, {-1, 2, 32}},
      {"ablate", 0, {4, 32}, {}},         {"S", 0, {0, 1, 64}, {-1, 65}},
      {"qres", -1, {-1, 0, 1}, {-2, 2}},   {"s3q", -1, {-1, 0, 1}, {-2, 2}},
      {"xhswz", 1, {0, 1}, {-1, 2}},      {"i8", -1, {-1, 0, 1}, {-2, 2}},
      {"i8w", -1, {-1, 0, 1}, {-2, 2}},    {"i8l1", -1, {-1, 0, 1, 2}, {-2, 3}},
      {"seed", 0, {-1, 0, 8192, 1ll << 40}, {-2}},
      {"s3gq", 0, {0, 1, 2, 4, 8, 16, 32}, {-1, 3, 64}},
      {"ophase", -1, {-1, 0, 64}, {-2, 65}}, {"order", -1, {-1, 0, 1, 2, 64}, {-2, 65}},
      {"qblk", 0, {0, 1, 1 << 20}, {-1, (1 << 20) + 1}},
      {"i8resc", -1, {-1, 0, 1}, {-2, 2}}, {"gg", -1, {-1, 4, 8}, {0, 2, 16}},
      {"nblk", -1, {-1, 0, 3}, {-2, 4}},   {"ties", 1, {0, 1, 2}, {-1, 3}},
      {"gk", -1, {-1, 0, 16}, {-2, 17}},
  };
  int pass = 0;
  for (const KeyValues& kv : keys) {
    const char* err = nullptr;
    for (int64_t v : kv.bad) {
      Tuning t;
      if (set_tuning(t, kv.key, v, &err) != KNN_ERR_ARG || !err || !strstr(err, kv.key)) {
        printf("VIOLATION tuning %s = %lld accepted or unexplained\n", kv.key, (long long)v);
        ++g_bad;
      }
    }
    for (int64_t v : kv.ok) {
      Tuning t;
      if (set_tuning(t, kv.key, v, &err) != KNN_OK) {
        printf("VIOLATION tuning %s = %lld refused\n", kv.key, (long long)v);
        ++g_bad;
        continue;
      }
      if (v == kv.def) continue;
      // (one fake build per setting, taking turns)
      static const int bl[] = {1, 2, 3, 4, 8};
      g_blocks = bl[pass % 5], g_qpw5 = pass & 1 ? 64 : 32, g_trows = pass & 2 ? 256 : 128;
      ++pass;
      walk(t, kv.key, v);
    }
  }
  {
    Tuning t;
    const char* err = "x";
    if (set_tuning(t, "nosuchkey", 0, &err) != KNN_ERR_ARG || err) {
      printf("VIOLATION unknown tuning key accepted\n");
      ++g_bad;
    }
  }
  printf("plan_check: %ld plans, %ld naming a kernel, %ld violations\n", g_plans, g_named, g_bad);
  return g_bad ? 1 : 0;
}
