// CPU check of ckb_zkp_amd/csrc/groth16_fold_plan.hpp against restatements of its definitions: the heavy-column cut, the column
// costs and C in column order on either side of the cut.  Prints "ok <cases checked>" or the first case that disagrees.
#include "groth16_fold_plan.hpp"

#include <cstdio>

using zkp::FoldCsc;

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rng() {                                          // xorshift64
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}

static long checked = 0;

// ---- fold_heavy_cut.  The definition: with `big` the costs above 1000 sorted descending, the candidates are "all heavy" (value
// 1000 + 150 |big|, threshold 1000) and, for each k < |big|, "the k largest heavy" (value big[k] + 150 k, threshold big[k]); the
// smallest value wins, on ties "all heavy" first, then the smallest k.
struct Candidate {
  uint64_t value;
  size_t order;
  uint64_t threshold;
};
static uint64_t cut_by_definition(std::vector<uint64_t> costs) {
  std::sort(costs.begin(), costs.end());
  std::vector<uint64_t> big;
  for (size_t i = costs.size(); i-- > 0;)
    if (costs[i] > 1000) big.push_back(costs[i]);
  std::vector<Candidate> cand;
  cand.push_back({1000 + 150 * (uint64_t)big.size(), 0, 1000});
  for (size_t k = 0; k < big.size(); k++) cand.push_back({big[k] + 150 * (uint64_t)k, k + 1, big[k]});
  const Candidate* best = &cand[0];
  for (const Candidate& c : cand)
    if (c.value < best->value || (c.value == best->value && c.order < best->order)) best = &c;
  return best->threshold;
}
static bool check_cut(const std::vector<uint64_t>& costs) {
  checked++;
  const uint64_t got = zkp::fold_heavy_cut(costs, 0), want = cut_by_definition(costs);
  if (got == want) return true;
  printf("fold_heavy_cut = %llu, definition = %llu for", (unsigned long long)got, (unsigned long long)want);
  for (size_t i = 0; i < costs.size() && i < 40; i++) printf(" %llu", (unsigned long long)costs[i]);
  printf(" (%zu costs)\n", costs.size());
  return false;
}
static const uint64_t EDGE_COSTS[9] = {0, 1, 999, 1000, 1001, 1150, 1151, 38000, 50000};
static bool exhaustive_cuts(std::vector<uint64_t>& costs, int left) {
  if (!check_cut(costs)) return false;
  if (left == 0) return true;
  for (uint64_t c : EDGE_COSTS) {
    costs.push_back(c);
    const bool ok = exhaustive_cuts(costs, left - 1);
    costs.pop_back();
    if (!ok) return false;
  }
  return true;
}
static size_t heavy_count(const std::vector<uint64_t>& costs, uint64_t cut) {
  size_t n = 0;
  for (uint64_t c : costs) n += c > cut;
  return n;
}
static bool expect(bool ok, const char* what) {
  checked++;
  if (!ok) printf("%s: not so\n", what);
  return ok;
}

// ---- fold_column_costs and fold_build_csc against a brute-force transpose of a small CSR matrix
static const uint64_t ONE[4] = {0x1111111111111111ull, 2, 3, 4}, MINUS_ONE[4] = {0x9999999999999999ull, 8, 7, 6};
struct Csr {
  size_t nz = 0;
  std::vector<uint32_t> row_ptr{0}, col;
  std::vector<uint64_t> coeff;                                   // 4 words per entry
  uint32_t rows() const { return (uint32_t)row_ptr.size() - 1; }
  int kind(size_t e) const { return memcmp(&coeff[4 * e], ONE, 32) == 0 ? 1 : memcmp(&coeff[4 * e], MINUS_ONE, 32) == 0 ? 2 : 0; }
};
static Csr random_csr(uint32_t rows, size_t nz, unsigned density) {           // an entry in density of 8 (row, variable) pairs, some twice
  Csr m;
  m.nz = nz;
  for (uint32_t k = 0; k < rows; k++) {
    for (size_t v = 0; v < nz; v++)
      for (int twice = 0; twice < 2; twice++) {
        if (rng() % 8 >= (twice ? density / 4 : density)) continue;
        m.col.push_back((uint32_t)((v * 7 + k) % nz));           // columns of a row in no particular order
        const unsigned which = (unsigned)(rng() % 3);
        for (int w = 0; w < 4; w++) m.coeff.push_back(which == 0 ? ONE[w] : which == 1 ? MINUS_ONE[w] : (rng() | 1) ^ (w == 3 ? 5 : 0));
      }
    m.row_ptr.push_back((uint32_t)m.col.size());
  }
  return m;
}
#define REQUIRE(cond)                                                              \
  if (!(cond)) {                                                                   \
    printf("line %d: %s (rows %u, nz %zu, nnz %zu, cut %llu)\n", __LINE__, #cond, m.rows(), m.nz, m.col.size(), (unsigned long long)cut); \
    return false;                                                                  \
  }
static bool check_csc(const Csr& m, int cut_choice) {
  checked++;
  const size_t nnz = m.col.size();
  uint64_t cut = 0;
  const std::vector<uint64_t> costs = zkp::fold_column_costs(m.nz, nnz, m.col.data(), m.coeff.data(), ONE, MINUS_ONE);
  REQUIRE(costs.size() == m.nz);
  for (size_t v = 0; v < m.nz; v++) {
    uint64_t want = 0;
    for (size_t e = 0; e < nnz; e++)
      if (m.col[e] == v) want += m.kind(e) ? 1 : 380;
    REQUIRE(costs[v] == want);
  }
  // every column with an entry heavy | none heavy | the per-key cut | a cost of the matrix (columns on either side of it)
  cut = cut_choice == 0 ? 0 : cut_choice == 1 ? UINT64_MAX : cut_choice == 2 ? zkp::fold_heavy_cut(costs, 0) : (m.nz ? costs[rng() % m.nz] : 7);
  FoldCsc c;
  REQUIRE(zkp::fold_build_csc(m.nz, m.rows(), m.row_ptr.data(), m.col.data(), m.coeff.data(), ONE, MINUS_ONE, costs, cut, &c));
  REQUIRE(c.col_ptr.size() == m.nz + 1 && c.col_ptr[0] == 0);
  REQUIRE(c.rows.size() == std::max<size_t>(nnz, 1) && c.kind.size() == c.rows.size() && c.coeff.size() == 8 * c.rows.size());
  REQUIRE(c.heavy.size() == c.heavy_cols.size());
  size_t light = 0, next_heavy = 0;
  for (size_t v = 0; v < m.nz; v++) {
    // the transpose, by brute force: the entries of variable v, rows ascending, a row's entries in their order
    std::vector<std::pair<uint32_t, uint32_t>> want;
    for (uint32_t k = 0; k < m.rows(); k++)
      for (uint32_t e = m.row_ptr[k]; e < m.row_ptr[k + 1]; e++)
        if (m.col[e] == v) want.emplace_back(k, e);
    if (costs[v] > cut) {
      REQUIRE(next_heavy < c.heavy_cols.size() && c.heavy_cols[next_heavy] == v);
      REQUIRE(c.heavy[next_heavy] == want);
      REQUIRE(c.col_ptr[v + 1] == c.col_ptr[v]);
      next_heavy++;
      continue;
    }
    REQUIRE(c.col_ptr[v] == light && c.col_ptr[v + 1] == light + want.size());          // the prefix sum of the light counts
    for (size_t j = 0; j < want.size(); j++) {
      const size_t pos = light + j, e = want[j].second;
      REQUIRE(c.rows[pos] == want[j].first && c.kind[pos] == m.kind(e));
      static const uint32_t zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      REQUIRE(memcmp(&c.coeff[8 * pos], m.kind(e) ? (const void*)zero : (const void*)&m.coeff[4 * e], 32) == 0);
    }
    light += want.size();
  }
  REQUIRE(next_heavy == c.heavy_cols.size());                    // the heavy lists hold exactly the rest
  if (cut_choice == 0) REQUIRE(light == 0);
  if (cut_choice == 1) REQUIRE(c.heavy_cols.empty() && light == nnz);
  // a column index >= nz anywhere is a failure
  if (nnz) {
    Csr bad = m;
    bad.col[rng() % nnz] = (uint32_t)(m.nz + rng() % 3);
    const std::vector<uint64_t> bad_costs = zkp::fold_column_costs(bad.nz, nnz, bad.col.data(), bad.coeff.data(), ONE, MINUS_ONE);
    REQUIRE(bad_costs.size() == m.nz);
    REQUIRE(!zkp::fold_build_csc(bad.nz, bad.rows(), bad.row_ptr.data(), bad.col.data(), bad.coeff.data(), ONE, MINUS_ONE, bad_costs, cut, &c));
  }
  return true;
}

int main() {
  std::vector<uint64_t> costs;
  if (!exhaustive_cuts(costs, 5)) return 1;                      // 1 + 9 + 9^2 + ... + 9^5 cost vectors
  // random vectors of up to 400 entries: costs on the grid 1000 + 150 j on which candidates tie, wide ones, and both mixed
  for (int it = 0; it < 4000; it++) {
    const size_t n = (size_t)(rng() % 401);
    costs.clear();
    for (size_t i = 0; i < n; i++) {
      const bool grid = it % 3 == 0 || (it % 3 == 1 && rng() % 2);
      costs.push_back(grid ? 850 + 150 * (rng() % (it % 2 ? 8 : 420)) : rng() % (it % 5 == 4 ? 3000 : 200000));
    }
    if (!check_cut(costs)) return 1;
  }
  bool ok = true;
  // the cases the comment at fold_heavy_cut names
  costs.assign(12, 38000);
  ok &= expect(heavy_count(costs, zkp::fold_heavy_cut(costs, 0)) == 12, "12 columns of 38 000 are all heavy");
  costs.assign(3000, 50000);
  ok &= expect(heavy_count(costs, zkp::fold_heavy_cut(costs, 0)) == 0, "3000 columns of 50 000: none heavy");
  ok &= expect(zkp::fold_heavy_cut(costs, 3) == 3 && zkp::fold_heavy_cut(costs, 50000) == 50000 && zkp::fold_heavy_cut({}, 77) == 77,
               "a positive fixed threshold is returned as given");
  ok &= expect(zkp::fold_heavy_cut({}, 0) == 1000, "no column: the floor");
  if (!ok) return 1;

  // the edges: no row, no variable, no entry
  for (int cut_choice = 0; cut_choice < 4; cut_choice++) {
    if (!check_csc(random_csr(0, 5, 4), cut_choice)) return 1;
    if (!check_csc(random_csr(6, 0, 4), cut_choice)) return 1;
    if (!check_csc(random_csr(7, 9, 0), cut_choice)) return 1;
  }
  for (int it = 0; it < 3000; it++) {
    const Csr m = random_csr((uint32_t)(rng() % 13), (size_t)(rng() % 11), (unsigned)(1 + rng() % 7));
    if (!check_csc(m, it % 4)) return 1;
  }
  printf("ok %ld\n", checked);
  return 0;
}
