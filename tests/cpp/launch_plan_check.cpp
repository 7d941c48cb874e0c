// CPU check of mad_icp_amd/csrc/common/launch_plan.h (tests/test_launch_plan.py compiles and runs it):
//   plan     every case of tests/golden/launch_plan/cases.json — recorded from the code BEFORE the header existed, as a table
//            of distinct results and an index per case — gives
//            the recorded grid, ranges per tree, qpt, LDS bytes, queue, interleave, route, flags_in_box, graph_ok (idle /
//            queued behind) and side_publish; the file must still cover every route, flag value, edge and option variation
//   key      plans that differ in one field give different graph keys, equal plans equal keys
//   options  every key of the table at the ends of its range and one step either side; the expected values and messages
//            are written out here, taken from the if-chains the table replaced
#include <cctype>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include <set>
#include <sstream>
#include <string>
#include <utility>
#include <vector>

#include "launch_plan.h"

using namespace madicp;

static int g_failures = 0;
#define CHECK(cond, ...)                                \
  do {                                                  \
    if (!(cond)) {                                      \
      if (++g_failures <= 20) {                         \
        std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); \
        std::printf(__VA_ARGS__);                       \
        std::printf("\n");                              \
      }                                                 \
    }                                                   \
  } while (0)

// ---- the little of JSON the fixture uses: objects, arrays, strings without escapes, integers -----------------------------------
struct Json {
  long long num = 0;
  std::string str;
  std::vector<Json> arr;
  std::vector<std::pair<std::string, Json>> obj;
  const Json& at(const std::string& k) const {
    for (const auto& kv : obj)
      if (kv.first == k) return kv.second;
    std::printf("FAIL fixture: no member \"%s\"\n", k.c_str());
    std::exit(1);
  }
  std::vector<int> ints() const {
    std::vector<int> v;
    for (const Json& e : arr) v.push_back((int)e.num);
    return v;
  }
};
struct Parser {
  const std::string& s;
  size_t i = 0;
  void ws() { while (i < s.size() && std::isspace((unsigned char)s[i])) ++i; }
  void expect(char c) {
    ws();
    if (i >= s.size() || s[i] != c) { std::printf("FAIL fixture: expected '%c' at byte %zu\n", c, i); std::exit(1); }
    ++i;
  }
  bool peek(char c) { ws(); return i < s.size() && s[i] == c; }
  std::string string() {
    expect('"');
    const size_t b = i;
    while (i < s.size() && s[i] != '"') ++i;
    return s.substr(b, i++ - b);
  }
  Json value() {
    Json v;
    ws();
    if (peek('{')) {
      ++i;
      while (!peek('}')) {
        std::string k = string();
        expect(':');
        v.obj.emplace_back(std::move(k), value());
        if (peek(',')) ++i;
      }
      ++i;
    } else if (peek('[')) {
      ++i;
      while (!peek(']')) {
        v.arr.push_back(value());
        if (peek(',')) ++i;
      }
      ++i;
    } else if (peek('"')) {
      v.str = string();
    } else {
      char* end = nullptr;
      v.num = std::strtoll(s.c_str() + i, &end, 10);
      if (end == s.c_str() + i) { std::printf("FAIL fixture: expected a value at byte %zu\n", i); std::exit(1); }
      i = end - s.c_str();
    }
    return v;
  }
};

// ---- plan ---------------------------------------------------------------------------------------------------------------------
static void check_plans(const std::string& path) {
  std::ifstream in(path);
  std::stringstream ss;
  ss << in.rdbuf();
  const std::string text = ss.str();
  CHECK(!text.empty(), "cannot read %s", path.c_str());
  if (text.empty()) return;
  Parser parser{text};
  const Json root = parser.value();
  const char* fields[] = {"grid", "ranges_per_tree", "qpt", "lds_bytes", "queue", "interleave", "route", "flags_in_box",
                          "graph_ok_idle", "graph_ok_queued_behind", "side_publish"};
  const char* routes[] = {"Rounds", "Persist", "Fold", "Tail", "P2p"};
  static_assert((int)Route::Rounds == 0 && (int)Route::Persist == 1 && (int)Route::Fold == 2 && (int)Route::Tail == 3 && (int)Route::P2p == 4,
                "the fixture numbers the routes in this order");
  const Json& jf = root.at("fields");
  CHECK(jf.arr.size() == 11, "fields");
  for (size_t f = 0; f < jf.arr.size() && f < 11; ++f) CHECK(jf.arr[f].str == fields[f], "field %zu is %s", f, jf.arr[f].str.c_str());
  const Json& jr = root.at("routes");
  CHECK(jr.arr.size() == 5, "routes");
  for (size_t r = 0; r < jr.arr.size() && r < 5; ++r) CHECK(jr.arr[r].str == routes[r], "route %zu is %s", r, jr.arr[r].str.c_str());

  const std::vector<Json>& rows = root.at("rows").arr;
  long n_cases = 0, seen_route[5] = {}, seen_flag[7][2] = {}, seen_qpt[3] = {};
  std::set<std::string> seen_variation;
  bool full_product = false, k0_sharded = false;
  const std::vector<int> Kfull{1, 7, 8, 9, 23, 24, 47, 48, 120, 121, 128};
  const std::vector<int> Lfull{1, 63, 64, 65, 255, 256, 1023, 1024, 1535, 1536, 16384, 131072, 131073, 524289};
  const std::vector<int> Bfull{1, 2, 3, 4, 8, 64}, Ifull{1, 2, 250, 251}, Tfull{0, 1};

  for (const Json& b : root.at("blocks").arr) {
    const std::string name = b.at("name").str;
    Options o;
    std::string variation;
    for (const auto& kv : b.at("options").obj) {
      std::string err;
      CHECK(option_set(o, kv.first, kv.second.num, &err), "%s: %s", name.c_str(), err.c_str());
      variation += kv.first + "=" + std::to_string(kv.second.num) + " ";
    }
    PlanEnv e;
    const Json& je = b.at("env");
    e.n_cus = (int)je.at("n_cus").num;
    e.rccl = je.at("rccl").num != 0;
    e.host_transport = je.at("host_transport").num != 0;
    e.p2p_attached = je.at("p2p_attached").num != 0;
    e.n_ranks = (int)je.at("n_ranks").num;
    if (e.rccl) variation += "rccl ";
    if (e.host_transport) variation += "host ";
    if (e.p2p_attached) variation += "attached ";
    seen_variation.insert(variation);
    const Json& ax = b.at("axes");
    const std::vector<int> aK = ax.at("K").ints(), aL = ax.at("max_L").ints(), aB = ax.at("batch").ints(), aI = ax.at("iters").ints(),
                           aT = ax.at("trace").ints(), aF = ax.at("flags_fit").ints();
    if (variation.empty() && e.n_cus == 256 && aK == Kfull && aL == Lfull && aB == Bfull && aI == Ifull && aT == Tfull) full_product = true;
    if (e.sharded() && e.n_cus == 256 && b.at("options").obj.empty() && aK == std::vector<int>{0} && aL == Lfull && aB == Bfull &&
        aI == Ifull && aT == Tfull)
      k0_sharded = true;
    std::string out;  // two base-36 digits per case: the index of its recorded tuple in "rows"
    for (const Json& piece : b.at("out").arr) out += piece.str;
    CHECK(out.size() == 2 * aK.size() * aL.size() * aB.size() * aI.size() * aT.size() * aF.size(), "%s: %zu digits", name.c_str(), out.size());
    size_t row = 0;
    for (int K : aK) for (int L : aL) for (int batch : aB) for (int iters : aI) for (int trace : aT) for (int fit : aF) {
      if (2 * row + 1 >= out.size()) return;
      auto digit = [](char c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'z' ? c - 'a' + 10 : 1 << 20; };
      const size_t at = (size_t)digit(out[2 * row]) * 36 + (size_t)digit(out[2 * row + 1]);
      ++row;
      if (at >= rows.size() || rows[at].arr.size() != 11) { CHECK(false, "%s: case %zu names no recorded tuple", name.c_str(), row - 1); continue; }
      const std::vector<int> want = rows[at].ints();
      if (!e.sharded() && K == 0) CHECK(false, "%s: K = 0 without a communicator", name.c_str());
      const Plan p = make_plan(o, e, L, K, batch, iters, trace != 0, fit != 0);
      const int got[11] = {p.grid, p.rpt, p.qpt, p.lds, p.queue, (int)p.interleave, (int)p.route, (int)p.flags_in_box,
                           (int)graph_ok(p, o, e, false, true), (int)graph_ok(p, o, e, true, true), (int)side_publish(p, o, e)};
      for (int f = 0; f < 11; ++f)
        CHECK(got[f] == want[f], "%s: K %d max_L %d batch %d iters %d trace %d flags_fit %d: %s is %d, recorded %d", name.c_str(), K, L,
              batch, iters, trace, fit, fields[f], got[f], want[f]);
      CHECK(p.batch == batch && p.iters == iters && p.K == K && p.trace == trace, "%s: the plan carries its inputs", name.c_str());
      CHECK(!graph_ok(p, o, e, false, false) && !graph_ok(p, o, e, true, false), "%s: a vetoed graph", name.c_str());
      ++n_cases;
      if (want[6] >= 0 && want[6] < 5) ++seen_route[want[6]];
      if (want[2] >= 1 && want[2] <= 2) ++seen_qpt[want[2]];
      const int flag_at[7] = {3, 4, 5, 7, 8, 9, 10};
      for (int f = 0; f < 7; ++f) ++seen_flag[f][want[flag_at[f]] != 0];
      if (e.p2p_attached && o.shard_p2p) seen_variation.insert(fit ? "flags fit" : "flags do not fit");
    }
  }
  // the fixture is still what it has to be
  CHECK(full_product, "no block holds the full product of the edges at default options");
  CHECK(k0_sharded, "no block holds K = 0 with a communicator at default options");
  for (int r = 0; r < 5; ++r) CHECK(seen_route[r] >= 50, "route %s in %ld cases only", routes[r], seen_route[r]);
  const char* flag_name[7] = {"lds_bytes", "queue", "interleave", "flags_in_box", "graph_ok_idle", "graph_ok_queued_behind", "side_publish"};
  for (int f = 0; f < 7; ++f)
    for (int v = 0; v < 2; ++v) CHECK(seen_flag[f][v] >= 50, "%s %s in %ld cases only", flag_name[f], v ? "set" : "clear", seen_flag[f][v]);
  CHECK(seen_qpt[1] >= 50 && seen_qpt[2] >= 50, "qpt 1 in %ld cases, 2 in %ld", seen_qpt[1], seen_qpt[2]);
  for (const char* v : {"persistent=1 ", "xcd_fold=1 ", "persistent=1 xcd_fold=1 ", "grid_blocks_per_cu=2 ", "grid_blocks_per_cu=4 ",
                        "units_per_workgroup=4 ", "queries_per_lane=2 ", "leaf_major=0 ", "deep_min_leaves=64 ", "lds_stage_min_leaves=0 ",
                        "lds_stage_min_leaves=1073741824 ", "interleave_ranges=0 ", "interleave_ranges=1 ", "rccl ", "shard_tail=1 rccl ",
                        "shard_p2p=1 rccl attached ", "shard_p2p=1 rccl ", "flags fit", "flags do not fit", "comm_graph=1 rccl ", "host "})
    CHECK(seen_variation.count(v) == 1, "no block for the variation '%s'", v);
  CHECK(n_cases >= 10000, "%ld cases", n_cases);
  std::printf("plans: %ld cases\n", n_cases);
}

// ---- key ----------------------------------------------------------------------------------------------------------------------
static bool differ(const GraphKey& a, const GraphKey& b) { return (a < b) != (b < a); }
static bool same(const GraphKey& a, const GraphKey& b) { return !(a < b) && !(b < a); }

static void check_keys() {
  Plan base;
  base.grid = 256; base.batch = 1; base.iters = 15; base.qpt = 1; base.lds = kTopLdsBytes; base.K = 16; base.rpt = 16;
  const GraphKey k0{base, 1, false};
  CHECK(same(k0, GraphKey{base, 1, false}), "equal plans, equal slots");
  std::vector<std::pair<const char*, Plan>> variants;
  auto vary = [&](const char* what, auto change) {
    Plan p = base;
    change(p);
    variants.emplace_back(what, p);
  };
  vary("grid", [](Plan& p) { p.grid = 248; });
  vary("batch", [](Plan& p) { p.batch = 2; });
  vary("iters", [](Plan& p) { p.iters = 14; });
  vary("qpt", [](Plan& p) { p.qpt = 2; });
  vary("lds", [](Plan& p) { p.lds = 0; });
  vary("K", [](Plan& p) { p.K = 17; });
  vary("rpt", [](Plan& p) { p.rpt = 32; });
  vary("trace", [](Plan& p) { p.trace = 1; });
  vary("queue", [](Plan& p) { p.queue = 1; });
  vary("flags_in_box", [](Plan& p) { p.flags_in_box = true; });
  vary("interleave", [](Plan& p) { p.interleave = true; });
  for (Route r : {Route::Persist, Route::Fold, Route::Tail, Route::P2p}) vary("route", [r](Plan& p) { p.route = r; });
  CHECK(variants.size() == 15, "one variant per field of Plan and per route");
  // (the key compares Plan::tie(), which lists the members next to their declarations; a member added there moves sizeof, and
  // this list has to be revisited)
  static_assert(sizeof(Plan) == 9 * sizeof(int) + sizeof(Route) + 4, "Plan has a field this check does not vary");
  for (const auto& v : variants) {
    CHECK(differ(k0, GraphKey{v.second, 1, false}), "a plan that differs in %s (route %d) has the key of the base plan", v.first, (int)v.second.route);
    CHECK(same(GraphKey{v.second, 2, true}, GraphKey{v.second, 2, true}), "equal plans (%s), equal keys", v.first);
  }
  for (size_t a = 0; a < variants.size(); ++a)  // the routes among themselves too
    for (size_t b = a + 1; b < variants.size(); ++b)
      CHECK(differ(GraphKey{variants[a].second, 0, true}, GraphKey{variants[b].second, 0, true}), "variants %zu and %zu share a key", a, b);
  Plan tail = base, rounds = base;
  tail.route = Route::Tail;
  rounds.route = Route::Rounds;
  CHECK(differ(GraphKey{tail, -1, true}, GraphKey{rounds, -1, true}), "Tail and Rounds share a key");
  CHECK(differ(k0, GraphKey{base, 2, false}), "slot");
  CHECK(differ(k0, GraphKey{base, 1, true}), "communicator");
  std::printf("keys ok\n");
}

// ---- options ------------------------------------------------------------------------------------------------------------------
struct Probe {
  long long value;
  bool accepted;
  long long stored;  // (accepted) what get returns afterwards
};
struct KeyExpect {
  const char* key;
  long long def;
  const char* refusal;  // the message of a refused value
  std::vector<Probe> probes;
};

static std::vector<Probe> boolean() { return {{-1, true, 1}, {0, true, 0}, {1, true, 1}, {2, true, 1}, {1ll << 40, true, 1}}; }

static void check_options() {
  const long long G = 1ll << 30;
  const std::vector<KeyExpect> expect = {
      {"grid_blocks_per_cu", 1, "grid_blocks_per_cu must be in 1..4", {{0, false, 0}, {1, true, 1}, {2, true, 2}, {3, true, 3}, {4, true, 4}, {5, false, 0}}},
      {"publish_side", 1, "", boolean()},
      {"deal_trees", 2, "deal_trees is 0 (as listed), 1 (round-robin over the XCD pieces) or 2 (alternating rows)",
       {{-1, false, 0}, {0, true, 0}, {1, true, 1}, {2, true, 2}, {3, false, 0}}},
      {"units_per_workgroup", 1, "units_per_workgroup must be in 1..64", {{0, false, 0}, {1, true, 1}, {2, true, 2}, {63, true, 63}, {64, true, 64}, {65, false, 0}}},
      {"use_graph", 1, "", boolean()},
      {"comm_graph", 0, "", boolean()},
      {"cache_correspondences", 1, "", boolean()},
      {"cache_gate", 1, "", boolean()},
      {"deep_min_leaves", 512, "deep_min_leaves must be in 64 .. 2^24",
       {{63, false, 0}, {64, true, 64}, {65, true, 65}, {16777215, true, 16777215}, {16777216, true, 16777216}, {16777217, false, 0}}},
      {"interleave_ranges", 2, "interleave_ranges is 0 (never), 1 (batches that share the chip) or 2 (always)",
       {{-1, false, 0}, {0, true, 0}, {1, true, 1}, {2, true, 2}, {3, false, 0}}},
      {"leaf_major", 8192, "leaf_major must be 0 (never) or a node count per pass",
       {{-1, false, 0}, {0, true, 0}, {1, true, 1}, {1048575, true, 1048575}, {1048576, true, 1048576}, {1048577, false, 0}}},
      {"lds_stage_min_leaves", 1024, "lds_stage_min_leaves must be >= 0",
       {{-1, false, 0}, {0, true, 0}, {1, true, 1}, {G - 1, true, G - 1}, {G, true, G}, {G + 1, true, G}, {1ll << 40, true, G}}},
      {"eager_when_busy", 1, "", boolean()},
      {"seq_completion", 1, "", boolean()},
      {"host_feed_wait", 1, "", boolean()},
      {"xcd_fold", 0, "", boolean()},
      {"debug_collective_us", 0, "", {{-1, true, 0}, {0, true, 0}, {1, true, 1}, {999, true, 999}, {1000, true, 1000}, {1001, true, 1000}}},
      {"shard_tail", 0, "", boolean()},
      {"build_after_registration", 0, "", boolean()},
      {"shard_p2p", 0, "", boolean()},
      {"shard_split", 1, "", {{-1, true, 0}, {0, true, 0}, {1, true, 1}, {2, true, 2}, {3, true, 2}, {1ll << 40, true, 2}}},
      {"match_all_rounds", 0, "", boolean()},
      {"persistent", 0, "", boolean()},
      {"wait_mode", 0, "wait_mode must be 0 (spin), 1 (yield) or 2 (sleep)", {{-1, false, 0}, {0, true, 0}, {1, true, 1}, {2, true, 2}, {3, false, 0}}},
      {"wait_timeout_ms", 0, "wait_timeout_ms must be >= 0",
       {{-1, false, 0}, {0, true, 0}, {1, true, 1}, {G - 1, true, G - 1}, {G, true, G}, {G + 1, true, G}}},
      {"comm_timeout_ms", 60000, "comm_timeout_ms must be >= 1",
       {{0, false, 0}, {1, true, 1}, {2, true, 2}, {G - 1, true, G - 1}, {G, true, G}, {G + 1, true, G}}},
      {"p2p_allow_coarse", 0, "", boolean()},
      {"upload_f32", 1, "", boolean()},
      {"nn_lds_top", 0, "", boolean()},
      {"queries_per_lane", 0, "queries_per_lane must be 0 (default), 1 or 2", {{-1, false, 0}, {0, true, 0}, {1, true, 1}, {2, true, 2}, {3, false, 0}}},
  };
  std::set<std::string> expected_keys;
  for (const KeyExpect& k : expect) expected_keys.insert(k.key);
  std::set<std::string> table_keys;
  for (const OptionRow& r : kOptionTable) table_keys.insert(r.name);
  CHECK(table_keys == expected_keys && table_keys.size() == sizeof(kOptionTable) / sizeof(kOptionTable[0]),
        "the table's keys are not the %zu keys this check knows", expected_keys.size());

  const Options defaults;
  for (const KeyExpect& k : expect) {
    int64_t got = 0;
    CHECK(option_get(defaults, k.key, &got) && got == k.def, "%s: default %lld, expected %lld", k.key, (long long)got, k.def);
    Options o;
    for (const Probe& p : k.probes) {
      int64_t before = 0, after = 0;
      option_get(o, k.key, &before);
      const Options copy = o;
      std::string err = "-";
      const bool ok = option_set(o, k.key, p.value, &err);
      option_get(o, k.key, &after);
      CHECK(ok == p.accepted, "%s = %lld: %s", k.key, p.value, ok ? "accepted" : "refused");
      if (p.accepted) {
        CHECK(after == p.stored, "%s = %lld: stored %lld, expected %lld", k.key, p.value, (long long)after, p.stored);
      } else {
        CHECK(after == before, "%s = %lld: a refused value changed the option to %lld", k.key, p.value, (long long)after);
        CHECK(err == k.refusal, "%s = %lld: message '%s'", k.key, p.value, err.c_str());
      }
      // nothing else moves
      for (const KeyExpect& other : expect) {
        int64_t a = 0, b = 0;
        option_get(copy, other.key, &a);
        option_get(o, other.key, &b);
        if (std::string(other.key) != k.key) CHECK(a == b, "%s = %lld moved %s", k.key, p.value, other.key);
      }
    }
  }
  for (const char* key : {"no_such_option", "", "p2p_fine_grained", "comm_ranks", "comm_rank"}) {
    Options o;
    std::string err;
    int64_t got = 77;
    CHECK(!option_set(o, key, 1, &err), "'%s' accepted", key);
    CHECK(err == std::string("unknown option: ") + key, "'%s': message '%s'", key, err.c_str());
    CHECK(!option_get(o, key, &got) && got == 77, "'%s' readable from the table", key);
  }
  std::printf("options ok\n");
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::printf("usage: launch_plan_check <cases.json>\n");
    return 2;
  }
  check_plans(argv[1]);
  check_keys();
  check_options();
  if (g_failures) {
    std::printf("%d failures\n", g_failures);
    return 1;
  }
  std::printf("launch plan ok\n");
  return 0;
}
