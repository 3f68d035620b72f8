// Stand-alone host check of csrc/allsteps_consts.h (built and run by tests/test_tree_plan.py, plain and
// with -fsanitize=address,undefined): plan_tree's words against their definitions, its rejections, and
// sweep_skip_mask on every accepted tree.
//
//   tree_plan_check [NAME NUM_LINKS PARENT,.. CFG_DOF_LINK,..]...
//
// The trees on the command line (the test passes the walker's and the quadruped's) join the program's
// own: a 17-link chain (the deepest the FK's four jump rounds reach), a star and a two-level binary tree.
// Every plan word is recomputed here from what it means, by walking parent[] link by link -- not by the
// builder's loops -- and compared with plan_tree's.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../allsteps_isaaclab_amd/csrc/allsteps_consts.h"

static int g_bad = 0;

static void expect(const char* tree, const char* what, int i, uint64_t got, uint64_t want) {
  if (got != want && g_bad++ < 20)
    std::printf("%s %s[%d]: got 0x%llx want 0x%llx\n", tree, what, i, (unsigned long long)got, (unsigned long long)want);
}

struct Tree {
  std::string name;
  std::vector<int> parent, cfg_dof_link;
};

static as::Consts make_consts(const Tree& t) {
  as::Consts c{};
  const int nl = (int)t.parent.size();
  c.model.num_links = nl;
  c.model.num_hinges = nl - 1;
  c.nv = 6 + nl - 1;
  for (int i = 0; i < nl && i < AS_MAX_LINKS; ++i) c.model.parent[i] = t.parent[i];
  for (int k = 0; k < (int)t.cfg_dof_link.size() && k < AS_MAX_LINKS; ++k) c.model.cfg_dof_link[k] = t.cfg_dof_link[k];
  return c;
}

// a is i or an ancestor of i
static bool on_path(const std::vector<int>& parent, int a, int i) {
  for (int x = i; x != -1; x = parent[x])
    if (x == a) return true;
  return false;
}
// the n-th ancestor of i, 0 past the root
static int ancestor(const std::vector<int>& parent, int i, int n) {
  int x = i;
  for (int s = 0; s < n; ++s) x = x > 0 ? parent[x] : 0;
  return x;
}
static int dof_link(int j) { return j < 6 ? 0 : j - 5; }

static void check_accepted(const Tree& t) {
  const char* name = t.name.c_str();
  const std::vector<int>& parent = t.parent;
  const int nl = (int)parent.size(), nv = 6 + nl - 1;
  as::Consts c = make_consts(t);
  // stale words must not survive a second plan
  std::memset(c.lpath, 0xff, sizeof(c.lpath));
  std::memset(c.ddesc, 0xff, sizeof(c.ddesc));
  c.root_kids = ~0u;
  c.max_path = c.max_sub = c.fk_rounds = 99;
  std::string err;
  if (!as::plan_tree(c, err)) {
    std::printf("%s: rejected (%s)\n", name, err.c_str());
    ++g_bad;
    return;
  }
  uint32_t lpath[as::kMaxLinks] = {}, lsub[as::kMaxLinks] = {}, ancmask[as::kMaxLinks] = {}, jump[as::kMaxLinks] = {};
  uint32_t root_kids = 0;
  int max_path = 0, max_sub = 0;
  for (int i = 0; i < nl; ++i) {
    int depth = 0, below = 0;
    ancmask[i] = 0x3Fu;
    for (int a = 0; a < nl; ++a) {
      if (on_path(parent, a, i)) {
        lpath[i] |= 1u << a;
        if (a != i) ++depth;
        if (a >= 1) ancmask[i] |= 1u << (6 + a - 1);
      }
      if (on_path(parent, i, a)) {
        lsub[i] |= 1u << a;
        if (a != i) ++below;
      }
    }
    for (int r = 0; r < 4; ++r) jump[i] |= (uint32_t)ancestor(parent, i, 1 << r) << (8 * r);
    if (parent[i] == 0) root_kids |= 1u << i;
    if (depth > max_path) max_path = depth;
    if (i > 0 && below > max_sub) max_sub = below;
  }
  int fk_rounds = 0;
  while ((1 << fk_rounds) < max_path) ++fk_rounds;
  for (int i = 0; i < as::kMaxLinks; ++i) {  // past num_links: zero
    expect(name, "lpath", i, c.lpath[i], lpath[i]);
    expect(name, "lsub", i, c.lsub[i], lsub[i]);
    expect(name, "ancmask", i, c.ancmask[i], ancmask[i]);
    expect(name, "jump", i, c.jump[i], jump[i]);
  }
  for (int j = 0; j < as::kMaxDofs; ++j) {  // past nv: zero
    uint32_t dsub = 0, ddesc = 0;
    if (j < nv) {
      dsub = lsub[dof_link(j)];
      for (int k = 0; k < nv; ++k)
        if ((ancmask[dof_link(k)] >> j) & 1u) ddesc |= 1u << k;
    }
    expect(name, "dsub", j, c.dsub[j], dsub);
    expect(name, "ddesc", j, c.ddesc[j], ddesc);
  }
  expect(name, "root_kids", 0, c.root_kids, root_kids);
  expect(name, "max_path", 0, (uint64_t)c.max_path, (uint64_t)max_path);
  expect(name, "max_sub", 0, (uint64_t)c.max_sub, (uint64_t)max_sub);
  expect(name, "fk_rounds", 0, (uint64_t)c.fk_rounds, (uint64_t)fk_rounds);

  // the structural sweep: the compiled skips hold for the trees they were compiled for; a chain has every
  // dof on one root path, so nothing is structurally zero
  const uint64_t skip = as::sweep_skip_mask(c.model);
  if (t.name == "walker") expect(name, "skip & kSweepSkip27", nv, skip & as::kSweepSkip27, as::kSweepSkip27);
  if (t.name == "quadruped") expect(name, "skip & kSweepSkip18", nv, skip & as::kSweepSkip18, as::kSweepSkip18);
  if (t.name.compare(0, 5, "chain") == 0) expect(name, "skip", nv, skip, 0ull);
}

static void check_rejected(const Tree& t, const char* want) {
  as::Consts c = make_consts(t);
  std::string err;
  if (as::plan_tree(c, err) || err != want) {
    std::printf("%s: %s, want rejection \"%s\"\n", t.name.c_str(), err.empty() ? "accepted" : err.c_str(), want);
    ++g_bad;
  }
}

static std::vector<int> csv(const char* s) {
  std::vector<int> v;
  for (const char* p = s; *p;) {
    char* end;
    const long x = std::strtol(p, &end, 10);
    if (end == p) break;  // not a number
    v.push_back((int)x);
    p = *end == ',' ? end + 1 : end;
  }
  return v;
}

static Tree chain(const char* name, int nl) {
  Tree t{name, {}, {}};
  for (int i = 0; i < nl; ++i) t.parent.push_back(i - 1);
  for (int k = 0; k < nl - 1; ++k) t.cfg_dof_link.push_back(nl - 1 - k);  // some permutation of 1..nl-1
  return t;
}

int main(int argc, char** argv) {
  std::vector<Tree> trees;
  for (int a = 1; a + 3 < argc; a += 4) {
    Tree t{argv[a], csv(argv[a + 2]), csv(argv[a + 3])};
    const int nl = std::atoi(argv[a + 1]);
    if (nl < 1 || nl > as::kMaxLinks || (int)t.parent.size() < nl || (int)t.cfg_dof_link.size() < nl - 1) {
      std::printf("%s: bad arguments\n", argv[a]);
      return 2;
    }
    t.parent.resize(nl);
    t.cfg_dof_link.resize(nl - 1);
    trees.push_back(t);
  }
  trees.push_back(chain("chain17", 17));
  trees.push_back(Tree{"star", {-1, 0, 0, 0, 0, 0, 0, 0, 0}, {1, 2, 3, 4, 5, 6, 7, 8}});
  trees.push_back(Tree{"binary", {-1, 0, 0, 1, 1, 2, 2}, {3, 1, 4, 2, 6, 5}});
  for (const Tree& t : trees) check_accepted(t);

  {  // the deepest accepted chain, by its numbers
    as::Consts c = make_consts(chain("chain17", 17));
    std::string err;
    if (!as::plan_tree(c, err) || c.max_path != 16 || c.fk_rounds != 4) {
      std::printf("chain17: max_path %d fk_rounds %d, want 16 and 4\n", c.max_path, c.fk_rounds);
      ++g_bad;
    }
  }
  check_rejected(chain("chain18", 18), "tree deeper than 16 links");
  Tree bad = trees.back();
  bad.name = "parent[0] = 0";
  bad.parent[0] = 0;
  check_rejected(bad, "parent not topological");
  bad = trees.back();
  bad.name = "parent[3] = 3";
  bad.parent[3] = 3;
  check_rejected(bad, "parent not topological");
  bad.name = "parent[3] = 5";
  bad.parent[3] = 5;
  check_rejected(bad, "parent not topological");
  bad = trees.back();
  bad.name = "parent[2] = -1";
  bad.parent[2] = -1;
  check_rejected(bad, "parent not topological");
  bad = trees.back();
  bad.name = "cfg_dof_link = 0";
  bad.cfg_dof_link[2] = 0;
  check_rejected(bad, "cfg_dof_link");
  bad.name = "cfg_dof_link = num_links";
  bad.cfg_dof_link[2] = 7;
  check_rejected(bad, "cfg_dof_link");

  std::printf("tree plan: %d trees, %d mismatches\n", (int)trees.size(), g_bad);
  return g_bad ? 1 : 0;
}
