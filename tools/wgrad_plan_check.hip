// wgrad_plan_check.hip -- the grouped weight-gradient planner (unit_amd/csrc/conv_wgrad_plan.hip) as a stand-alone host program, so that
// it can run under AddressSanitizer / UBSan. No GPU, no Python: it links conv_wgrad_plan.hip alone.
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined tools/wgrad_plan_check.hip \
//         unit_amd/csrc/conv_wgrad_plan.hip -o wgrad_plan_check && ./wgrad_plan_check
// (tests/test_wgrad_plan_program_cpu.py does exactly that). It plans the problem lists of tests/golden/gen_wgrad_layout_parent.py at the six
// dealing modes, checks on every layout that each tile of each (layer [, filter tap], split) is there exactly once and that an XCD's slots
// are gap-free from 0, and asks for every refusal. Exit status 0 and nothing on stderr = fine.
#include <algorithm>
#include <map>
#include <string>
#include <tuple>
#include <vector>
#include "../unit_amd/csrc/conv_wgrad_host.h"

static const char* last_error = "";
extern "C" void unit_set_error(const char* msg) { last_error = msg; }
extern "C" int unit_conv2d_wgrad_group_plan(UnitWgradProblem* pr, int n, int splits_hint);
extern "C" int unit_conv2d_wgrad_group_layout(const UnitWgradProblem* pr, int n, int* layout, int layout_rows, int* rows);

static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { ++failures; fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); } } while (0)

struct Layer { int n, h, w, c, k, r, stride, pad; };
static const Layer SMALL_3X3 = {64, 7, 7, 256, 256, 3, 1, 1};

static std::vector<Layer> layers_of(const std::string& which) {
  std::vector<Layer> L;
  auto add = [&](std::initializer_list<Layer> ls, int times = 1) { for (int i = 0; i < times; ++i) L.insert(L.end(), ls); };
  if (which == "res5") {
    add({{1024, 14, 14, 1024, 512, 1, 2, 0}, {1024, 7, 7, 512, 512, 3, 1, 1}, {1024, 7, 7, 512, 2048, 1, 1, 0}, {1024, 14, 14, 1024, 2048, 1, 2, 0}});
    add({{1024, 7, 7, 2048, 512, 1, 1, 0}, {1024, 7, 7, 512, 512, 3, 1, 1}, {1024, 7, 7, 512, 2048, 1, 1, 0}}, 2);
  } else if (which == "res4" || which == "long") {
    add({{4, 38, 63, 1024, 256, 1, 1, 0}, {4, 38, 63, 256, 256, 3, 1, 1}, {4, 38, 63, 256, 1024, 1, 1, 0}}, which == "long" ? 9 : 6);
  } else if (which == "res3") {
    add({{4, 150, 250, 256, 128, 1, 2, 0}, {4, 75, 125, 128, 128, 3, 1, 1}, {4, 75, 125, 128, 512, 1, 1, 0}, {4, 150, 250, 256, 512, 1, 2, 0}});
    add({{4, 75, 125, 512, 128, 1, 1, 0}, {4, 75, 125, 128, 128, 3, 1, 1}, {4, 75, 125, 128, 512, 1, 1, 0}}, 3);
  } else if (which == "chunk2") {
    add({{64, 7, 7, 2048, 2048, 1, 1, 0}, {64, 7, 7, 512, 512, 3, 1, 1}});
  } else if (which == "chunk1") {
    add({{1, 20, 20, 384, 384, 3, 1, 1}, {1, 20, 20, 128, 128, 1, 1, 0}});
  } else if (which == "mixed") {
    L = layers_of("res4");
    for (const Layer& l : layers_of("res3")) L.push_back(l);
  } else {
    add({SMALL_3X3}, which == "full" ? 20 : which == "full2" ? 11 : 1);
  }
  return L;
}

static std::vector<UnitWgradProblem> problems(const std::vector<Layer>& L) {
  std::vector<UnitWgradProblem> pr;
  for (const Layer& l : L) {
    UnitWgradProblem q = {};
    q.x = (const void*)0x10000; q.dy = (const void*)0x20000; q.partial = (void*)0x30000;          // aligned, never read
    q.N = l.n; q.H = l.h; q.W = l.w; q.C = l.c; q.K = l.k; q.R = q.S = l.r; q.stride = l.stride; q.pad = l.pad;
    q.OH = (l.h + 2 * l.pad - l.r) / l.stride + 1; q.OW = (l.w + 2 * l.pad - l.r) / l.stride + 1; q.ldy = l.k;
    pr.push_back(q);
  }
  return pr;
}

static std::vector<UnitWgradProblem> planned(const std::string& which, int hint) {
  std::vector<UnitWgradProblem> pr = problems(layers_of(which));
  EXPECT(unit_conv2d_wgrad_group_plan(pr.data(), (int)pr.size(), hint) == UNIT_OK, "%s: %s", which.c_str(), last_error);
  if (which == "full" || which == "full2" || which == "tight")
    for (UnitWgradProblem& q : pr) {
      q.splits = which == "full" ? 1 : which == "full2" ? 2 : 21;
      if (which == "tight") q.kind = 2;
    }
  return pr;
}

static void set_mode(const char* gang, const char* deal) {
  if (gang) setenv("UNIT_WGRAD_GANG", gang, 1); else unsetenv("UNIT_WGRAD_GANG");
  if (deal) setenv("UNIT_WGRAD_DEAL", deal, 1); else unsetenv("UNIT_WGRAD_DEAL");
}

struct Row { int launch, kind, xcd, start, tiles, prob, tap, split, tile0; };
static_assert(sizeof(Row) == 9 * sizeof(int), "a layout row is 9 ints");
static bool in_map_3x3(const UnitWgradProblem& q) { return q.kind == 2 && q.R == 3 && q.stride == 1 && q.pad == 1 && q.OH * q.OW <= 512; }

// every tile exactly once, an XCD's units of one launch tile its slot range from 0 without gaps or overlaps
static std::vector<Row> check_layout(const std::string& what, const std::vector<UnitWgradProblem>& pr) {
  std::vector<Row> rows(4096);
  int n = 0;
  int st = unit_conv2d_wgrad_group_layout(pr.data(), (int)pr.size(), &rows[0].launch, (int)rows.size(), &n);
  EXPECT(st == UNIT_OK && n > 0, "%s: status %d (%s), %d rows", what.c_str(), st, last_error, n);
  rows.resize(st == UNIT_OK ? n : 0);
  std::map<std::tuple<int, int, int, int>, int> seen;
  std::map<std::pair<int, int>, std::vector<Row>> by;
  for (const Row& u : rows) {
    bool ok = u.prob >= 0 && u.prob < (int)pr.size() && u.xcd >= 0 && u.xcd < 8 && u.tiles > 0;
    EXPECT(ok, "%s: row out of range", what.c_str());
    if (!ok) continue;
    const UnitWgradProblem& q = pr[u.prob];
    EXPECT(u.kind == q.kind && u.split >= 0 && u.split < q.splits && (u.tap == 0 || (in_map_3x3(q) && u.tap < 9)), "%s: unit of layer %d", what.c_str(), u.prob);
    for (int t = u.tile0; t < u.tile0 + u.tiles; ++t) ++seen[{u.prob, u.tap, u.split, t}];
    by[{u.launch, u.xcd}].push_back(u);
  }
  size_t want = 0;
  for (int i = 0; i < (int)pr.size(); ++i) {
    const UnitWgradProblem& q = pr[i];
    const int T = q.kind == 2 ? 256 : 128, tiles = (q.R * q.S * q.C / T) * (q.K / T), taps = in_map_3x3(q) ? 9 : 1;
    for (int tap = 0; tap < taps; ++tap)
      for (int s = 0; s < q.splits; ++s)
        for (int t = 0; t < tiles / taps; ++t, ++want) {
          auto it = seen.find({i, tap, s, t});
          EXPECT(it != seen.end() && it->second == 1, "%s: layer %d tap %d split %d tile %d", what.c_str(), i, tap, s, t);
        }
  }
  EXPECT(seen.size() == want, "%s: %zu tiles for %zu", what.c_str(), seen.size(), want);
  for (auto& kv : by) {
    std::vector<Row>& us = kv.second;
    std::sort(us.begin(), us.end(), [](const Row& a, const Row& b) { return a.start < b.start; });
    EXPECT(us[0].start == 0, "%s: launch %d XCD %d starts at %d", what.c_str(), kv.first.first, kv.first.second, us[0].start);
    for (size_t i = 1; i < us.size(); ++i)
      EXPECT(us[i - 1].start + us[i - 1].tiles == us[i].start, "%s: launch %d XCD %d gap", what.c_str(), kv.first.first, kv.first.second);
    EXPECT(us.size() <= (size_t)WG_GROUP_MAX_UNITS, "%s: %zu units on one XCD", what.c_str(), us.size());
  }
  return rows;
}

static void expect_refused(const char* name, std::vector<UnitWgradProblem> pr, int cap = 4096, int want = UNIT_ERR_ARG) {
  std::vector<int> buf(9 * 4096);
  int n = -1;
  last_error = "";
  int st = unit_conv2d_wgrad_group_layout(pr.data(), (int)pr.size(), buf.data(), cap, &n);
  EXPECT(st == want && (st == UNIT_OK ? n == 0 : last_error[0] != 0), "%s: status %d, %d rows, \"%s\"", name, st, n, last_error);
}

int main() {
  static const struct { const char* which; int hint; } CASES[] = {{"res5", 0}, {"res5", 4}, {"res4", 0}, {"res4", 3}, {"res3", 0}, {"long", 0},
    {"chunk2", 0}, {"chunk1", 0}, {"mixed", 0}, {"full", 0}, {"full2", 0}, {"tight", 0}};
  static const struct { const char* gang; const char* deal; } MODES[] = {{nullptr, nullptr}, {"0", nullptr}, {"1", nullptr}, {"2", "0"}, {"0", "1"}, {"1", "0"}};
  for (const auto& c : CASES)
    for (const auto& m : MODES) {
      set_mode(m.gang, m.deal);
      const std::string what = std::string(c.which) + " hint " + std::to_string(c.hint) + " gang " + (m.gang ? m.gang : "-") + " deal " + (m.deal ? m.deal : "-");
      std::vector<UnitWgradProblem> pr = planned(c.which, c.hint);
      std::vector<Row> first = check_layout(what, pr), again = check_layout(what + " (again)", pr);          // the second call: the cached table
      EXPECT(first.size() == again.size() && (first.empty() || memcmp(first.data(), again.data(), first.size() * sizeof(Row)) == 0), "%s: the repeat differs", what.c_str());
    }
  set_mode(nullptr, nullptr);
  auto one = [](Layer l, int kind, int splits) {
    std::vector<UnitWgradProblem> pr = problems({l});
    pr[0].kind = kind; pr[0].splits = splits;
    return pr;
  };
  const Layer pw = {64, 7, 7, 256, 256, 1, 1, 0};
  std::vector<UnitWgradProblem> q;
  expect_refused("splits 0", one(pw, 2, 0));
  expect_refused("splits 128", one(pw, 2, 128));
  q = one(pw, 2, 2); q[0].x = (const void*)0x10008; expect_refused("misaligned x", q);
  q = one(pw, 2, 2); q[0].x_pitch = 128; expect_refused("x_pitch < C", q);
  q = one(pw, 2, 2); q[0].N = 0; expect_refused("N = 0", q);
  expect_refused("kind 0", one(pw, 0, 2), 4096, UNIT_OK);          // belongs to no grid: nothing planned, nothing refused
  expect_refused("kind 2, C = 384", one({64, 7, 7, 384, 384, 1, 1, 0}, 2, 2));
  expect_refused("tight, splits 22", one(SMALL_3X3, 2, 22));
  expect_refused("one row short", planned("tight", 0), 188);
  if (failures) fprintf(stderr, "%d checks failed\n", failures);
  return failures ? 1 : 0;
}
