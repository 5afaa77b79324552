// Stand-alone host program (test fixture, never shipped): drives the GEMM
// launch policy (marlin_amd/csrc/gemm_launch_policy.h) without a GPU.
//
//   (no argument)   knob decoding on a table of strings, then the selection
//                   invariants over a sweep of knobs, types, forms, shapes
//                   and pitches, then the size of the closed list
//   --list          the closed list of instantiations, one per line, in the
//                   spelling of the demangled kernel names:
//                   T,BETA,BK,BM,WM,WN,PIPE,TA,TB,EPI,GRP
//   --select NAME=VALUE ... CASE ...
//                   one JSON line per case under that knob set. CASE is
//                   fp32,beta,ta,tb,M,N,K[,lda,ldb] for the plain entry
//                   (pitches default to the stored leading dimensions) or
//                   g:fp32,beta,ta,tb,nbn0 for a grouped launch whose first
//                   table entry has nbn0 block columns.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <tuple>
#include <vector>

#include "gemm_launch_policy.h"

static int g_checks = 0;
#define REQUIRE(x)                                                    \
  do {                                                                \
    g_checks++;                                                       \
    if (!(x)) {                                                       \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #x);             \
      return 1;                                                       \
    }                                                                 \
  } while (0)

typedef std::map<std::string, std::string> env_t;

static mx_gemm_knobs parse(const env_t& env) {
  return mx_gemm_parse_knobs([&](const char* name) -> const char* {
    auto it = env.find(name);
    return it == env.end() ? nullptr : it->second.c_str();
  });
}

static const char* const KNOB_NAMES[5] = {
    "MARLIN_GEMM_BAND", "MARLIN_GEMM_REMAP", "MARLIN_GEMM_CFG",
    "MARLIN_GEMM_PHASE", "MARLIN_GEMM_LOOP"};

// every string in every knob, the other four unset
static int check_decoding() {
  struct row { const char* s; int band, plain, geom, phase, loop; };
  const row rows[] = {
      // string    band plain geometry         phase loop
      {nullptr,    8,   0,    MX_GEOM_DEFAULT, 0,    MX_LOOP_UNSET},
      {"",         8,   0,    MX_GEOM_DEFAULT, 0,    MX_LOOP_UNSET},
      {"0",        8,   0,    MX_GEOM_DEFAULT, 0,    MX_LOOP_UNSET},
      {"-3",       8,   0,    MX_GEOM_DEFAULT, -3,   MX_LOOP_UNSET},
      {"4",        4,   0,    MX_GEOM_DEFAULT, 4,    MX_LOOP_UNSET},
      {"16",       16,  0,    MX_GEOM_DEFAULT, 16,   MX_LOOP_UNSET},
      {"bands",    8,   1,    MX_GEOM_DEFAULT, 0,    MX_LOOP_UNSET},
      {"bk32",     8,   1,    MX_GEOM_BK32,    0,    MX_LOOP_UNSET},
      {"bm256",    8,   1,    MX_GEOM_BM256,   0,    MX_LOOP_UNSET},
      {"b",        8,   1,    MX_GEOM_DEFAULT, 0,    MX_LOOP_UNSET},
      {"twobar",   8,   0,    MX_GEOM_DEFAULT, 0,    MX_LOOP_TWOBAR},
      {"pipe",     8,   0,    MX_GEOM_DEFAULT, 0,    MX_LOOP_PIPE},
      {"x",        8,   0,    MX_GEOM_DEFAULT, 0,    MX_LOOP_UNSET},
  };
  const mx_gemm_knobs unset = parse({});
  for (const row& r : rows) {
    for (int which = 0; which < 5; which++) {
      env_t env;
      if (r.s) env[KNOB_NAMES[which]] = r.s;
      const mx_gemm_knobs k = parse(env);
      REQUIRE(k.band_width == (which == 0 ? r.band : unset.band_width));
      REQUIRE(k.plain_bands == (which == 1 ? r.plain : unset.plain_bands));
      REQUIRE(k.geometry == (which == 2 ? r.geom : unset.geometry));
      REQUIRE(k.phase_mask == (which == 3 ? r.phase : unset.phase_mask));
      REQUIRE(k.loop == (which == 4 ? r.loop : unset.loop));
      REQUIRE(k.band_width >= 1);
    }
  }
  return 0;
}

typedef std::tuple<int, int, int, int, int, int, int, int, int, int, int> vkey;
static vkey key_of(const mx_gemm_variant& v) {
  return vkey(v.T, v.BETA, v.BK, v.BM, v.WM, v.WN, v.PIPE, v.TA, v.TB, v.EPI,
               v.GRP);
}

static int check_selection(int* points) {
  std::set<vkey> list, reached;
  for (const mx_gemm_variant& v : mx_gemm_instantiations())
    list.insert(key_of(v));
  REQUIRE(list.size() == 77);                       // 77 distinct members
  REQUIRE(mx_gemm_instantiations().size() == 77);

  const int64_t BOUND = (int64_t)1 << 26;           // restated on purpose
  REQUIRE(MX_GEMM_PITCH32_BOUND == BOUND);
  const char* const geoms[] = {nullptr, "bk32", "bm256"};
  const char* const loops[] = {nullptr, "twobar", "pipe"};
  for (int gi = 0; gi < 3; gi++)
  for (int li = 0; li < 3; li++) {
    env_t env;
    if (geoms[gi]) env["MARLIN_GEMM_CFG"] = geoms[gi];
    if (loops[li]) env["MARLIN_GEMM_LOOP"] = loops[li];
    const mx_gemm_knobs kn = parse(env);
    for (int fp32 = 0; fp32 < 2; fp32++)
    for (int beta = 0; beta < 2; beta++)
    for (int ta = 0; ta < 2; ta++)
    for (int tb = 0; tb < 2; tb++) {
      for (int64_t M : {128, 256, 384})
      for (int64_t K : {16, 32, 48})
      for (int64_t lda : {BOUND - 4, BOUND})
      for (int64_t ldb : {BOUND - 4, BOUND}) {
        const mx_gemm_variant v =
            mx_gemm_select(kn, fp32, beta, ta, tb, M, 1152, K, lda, ldb);
        (*points)++;
        REQUIRE(list.count(key_of(v)) == 1);
        reached.insert(key_of(v));
        REQUIRE(v.T == fp32 && v.BETA == beta && v.TA == ta && v.TB == tb);
        REQUIRE(v.EPI == 0 && v.GRP == 0);
        const bool dflt = v.BK == 16 && v.BM == 128 && v.WM == 2 && v.WN == 2;
        if (ta || tb) REQUIRE(dflt);
        if (fp32) REQUIRE(v.BM == 128);
        // the geometry rule, restated
        const bool nn = !ta && !tb;
        REQUIRE((v.BK == 32) == (nn && gi == 1 && K % 32 == 0));
        REQUIRE((v.BM == 256) == (nn && gi == 2 && !fp32 && M % 256 == 0));
        REQUIRE(v.WM * v.WN == (dflt ? 4 : 8));
        REQUIRE(M % v.BM == 0 && K % v.BK == 0);
        // the loop rule, restated
        const bool below = lda < BOUND && ldb < BOUND;
        if (!below) REQUIRE(v.PIPE == 0);
        else if (li) REQUIRE(v.PIPE == (li == 2));
        else REQUIRE(v.PIPE == !(fp32 && v.BK == 16));
        REQUIRE(v.band == 8 && v.phase_mask == 0);  // nbn = 9, no knob
      }
      for (int p32 = 0; p32 < 2; p32++) {
        const mx_gemm_variant v =
            mx_gemm_select_grouped(kn, fp32, beta, ta, tb, 2, p32 != 0);
        (*points)++;
        REQUIRE(list.count(key_of(v)) == 1);
        reached.insert(key_of(v));
        REQUIRE(v.T == fp32 && v.BETA == beta && v.TA == ta && v.TB == tb);
        REQUIRE(v.BK == 16 && v.BM == 128 && v.WM == 2 && v.WN == 2);
        REQUIRE(v.EPI == 0 && v.GRP == 1 && v.band == 2 && v.phase_mask == 0);
        if (!p32) REQUIRE(v.PIPE == 0);
        else if (li) REQUIRE(v.PIPE == (li == 2));
        else REQUIRE(v.PIPE == !fp32);
      }
    }
  }
  // the fused epilogue is fixed, and the last member the sweep must reach
  for (int64_t nbn : {1, 3, 8, 9, 17}) {
    const mx_gemm_variant v = mx_gemm_select_epilogue(128 * nbn);
    (*points)++;
    REQUIRE(key_of(v) == vkey(1, 0, 16, 128, 2, 2, 0, 0, 0, 1, 0));
    REQUIRE(v.band == (nbn < 8 ? nbn : 8) && v.phase_mask == 0);
    reached.insert(key_of(v));
  }
  REQUIRE(reached == list);                 // no member is dead either
  // band and phase follow their knobs
  { env_t env = {{"MARLIN_GEMM_BAND", "3"}, {"MARLIN_GEMM_REMAP", "bands"},
                 {"MARLIN_GEMM_PHASE", "8"}};
    const mx_gemm_knobs kn = parse(env);
    REQUIRE(mx_gemm_select(kn, 0, 0, 0, 0, 128, 1152, 16, 128, 16).band == -3);
    REQUIRE(mx_gemm_select(kn, 0, 0, 0, 0, 128, 256, 16, 128, 16).band == -2);
    REQUIRE(mx_gemm_select(kn, 1, 1, 1, 0, 128, 256, 16, 16, 16).phase_mask == 8);
    REQUIRE(mx_gemm_band(kn, 1) == -1); }
  // pitch contract
  REQUIRE(pitch_ok(128, 128, 2) && !pitch_ok(126, 128, 2));
  REQUIRE(!pitch_ok(129, 128, 2) && pitch_ok(130, 128, 2) && !pitch_ok(130, 128, 4));
  return 0;
}

static void print_key(const mx_gemm_variant& v) {
  printf("%s,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d\n", v.T ? "float" : "double",
         v.BETA, v.BK, v.BM, v.WM, v.WN, v.PIPE, v.TA, v.TB, v.EPI, v.GRP);
}

static int select_mode(int argc, char** argv) {
  env_t env;
  int i = 2;
  for (; i < argc && strchr(argv[i], '='); i++) {
    const std::string a = argv[i];
    env[a.substr(0, a.find('='))] = a.substr(a.find('=') + 1);
  }
  const mx_gemm_knobs kn = parse(env);
  for (; i < argc; i++) {
    const char* s = argv[i];
    const bool grouped = s[0] == 'g' && s[1] == ':';
    std::vector<int64_t> f;
    for (const char* p = grouped ? s + 2 : s; *p;) {
      char* end;
      f.push_back(strtoll(p, &end, 10));
      if (end == p || (*end && *end != ',')) return 2;
      p = *end ? end + 1 : end;
    }
    mx_gemm_variant v;
    if (grouped) {
      if (f.size() != 5) return 2;
      v = mx_gemm_select_grouped(kn, (int)f[0], (int)f[1], (int)f[2],
                                 (int)f[3], mx_gemm_band(kn, f[4]), true);
    } else {
      if (f.size() != 7 && f.size() != 9) return 2;
      const int64_t M = f[4], N = f[5], K = f[6];
      const int64_t lda = f.size() == 9 ? f[7] : (f[2] ? K : M);
      const int64_t ldb = f.size() == 9 ? f[8] : (f[3] ? N : K);
      v = mx_gemm_select(kn, (int)f[0], (int)f[1], (int)f[2], (int)f[3], M, N,
                         K, lda, ldb);
    }
    printf("{\"is_fp32\": %d, \"beta_one\": %d, \"bk\": %d, \"bm\": %d, "
           "\"waves\": %d, \"band\": %d, \"phase_mask\": %d, \"loop\": %d, "
           "\"op\": [%d, %d], \"grouped\": %d}\n",
           v.T, v.BETA, v.BK, v.BM, v.WM * v.WN, v.band, v.phase_mask, v.PIPE,
           v.TA, v.TB, v.GRP);
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "--list")) {
    for (const mx_gemm_variant& v : mx_gemm_instantiations()) print_key(v);
    return 0;
  }
  if (argc > 1 && !strcmp(argv[1], "--select")) return select_mode(argc, argv);
  int points = 0;
  if (check_decoding()) return 1;
  if (check_selection(&points)) return 1;
  printf("gemm_launch_policy OK %d points %d checks\n", points, g_checks);
  return 0;
}
