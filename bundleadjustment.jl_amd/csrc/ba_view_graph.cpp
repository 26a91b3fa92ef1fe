// Host-only: the view graph of rotation averaging -- the argument checks on the pair list, the CSR adjacency the kernels of
// ba_rotavg_kernels.hip read, and the maximum spanning forest (ba_view_graph_forest; include/ba_hip.h, "rotation averaging";
// DESIGN §5u).  No HIP, no device: a CPU test calls the entry.
#include "ba_view_graph.h"

#include <algorithm>
#include <cmath>
#include <numeric>

#include "../../include/ba_hip.h"

void ba_set_error(const char *fmt, ...);

int view_graph_check(const char *who, int64_t ncams, int64_t npairs, const int64_t *pair_a1, const int64_t *pair_b1) {
  if (ncams < 0 || npairs < 0 || (npairs > 0 && (!pair_a1 || !pair_b1))) {
    ba_set_error("%s: null argument or a negative size", who);
    return 1;
  }
  if (ncams >= INT32_MAX || npairs >= (int64_t)1 << 30) {
    ba_set_error("%s: %lld cameras, %lld pairs: more than the 32-bit tables hold", who, (long long)ncams, (long long)npairs);
    return 1;
  }
  std::vector<uint64_t> key((size_t)npairs);
  for (int64_t k = 0; k < npairs; k++) {
    const int64_t a = pair_a1[k], b = pair_b1[k];
    if (a < 1 || a > ncams || b < 1 || b > ncams) {
      ba_set_error("%s: pair %lld = (%lld, %lld): 1-based cameras must lie in 1..%lld", who, (long long)k, (long long)a, (long long)b,
                   (long long)ncams);
      return 1;
    }
    if (a == b) {
      ba_set_error("%s: pair %lld holds camera %lld twice: a pair holds two different cameras", who, (long long)k, (long long)a);
      return 1;
    }
    key[(size_t)k] = (uint64_t)std::min(a, b) * (uint64_t)(ncams + 1) + (uint64_t)std::max(a, b);
  }
  std::sort(key.begin(), key.end());
  for (int64_t k = 1; k < npairs; k++)
    if (key[(size_t)k] == key[(size_t)k - 1]) {
      ba_set_error("%s: the pair of cameras (%lld, %lld) is listed twice", who, (long long)(key[(size_t)k] / (uint64_t)(ncams + 1)),
                   (long long)(key[(size_t)k] % (uint64_t)(ncams + 1)));
      return 1;
    }
  return 0;
}

void view_graph_csr(int64_t ncams, int64_t npairs, const int64_t *pair_a1, const int64_t *pair_b1, const uint8_t *mask,
                    std::vector<int> *ptr, std::vector<int> *nbr, std::vector<int> *edge) {
  ptr->assign((size_t)ncams + 1, 0);
  for (int64_t k = 0; k < npairs; k++)
    if (!mask || mask[k]) (*ptr)[(size_t)pair_a1[k]]++, (*ptr)[(size_t)pair_b1[k]]++;  // (1-based camera c counts into ptr[c])
  for (int64_t c = 0; c < ncams; c++) (*ptr)[(size_t)c + 1] += (*ptr)[(size_t)c];
  const size_t n = (size_t)(*ptr)[(size_t)ncams];
  std::vector<int64_t> ent(n);  // neighbour << 31 | edge: sorting the entries of a camera sorts them by neighbour
  std::vector<int> fill(ptr->begin(), ptr->end() - 1);
  for (int64_t k = 0; k < npairs; k++)
    if (!mask || mask[k]) {
      const int64_t a = pair_a1[k] - 1, b = pair_b1[k] - 1;
      ent[(size_t)fill[(size_t)a]++] = (b << 31) | (2 * k);
      ent[(size_t)fill[(size_t)b]++] = (a << 31) | (2 * k + 1);
    }
  nbr->resize(n);
  edge->resize(n);
  for (int64_t c = 0; c < ncams; c++) {
    std::sort(ent.begin() + (*ptr)[(size_t)c], ent.begin() + (*ptr)[(size_t)c + 1]);
    for (int e = (*ptr)[(size_t)c]; e < (*ptr)[(size_t)c + 1]; e++) {
      (*nbr)[(size_t)e] = (int)(ent[(size_t)e] >> 31);
      (*edge)[(size_t)e] = (int)(ent[(size_t)e] & 0x7fffffff);
    }
  }
}

namespace {
int find_root(std::vector<int> &up, int c) {
  while (up[(size_t)c] != c) c = up[(size_t)c] = up[(size_t)up[(size_t)c]];
  return c;
}
}  // namespace

void view_graph_forest(int64_t ncams, int64_t npairs, const int64_t *pair_a1, const int64_t *pair_b1, const uint8_t *used,
                       const int32_t *support, const double *weights, const uint8_t *fixed, ViewForest *out) {
  const size_t nc = (size_t)ncams;
  // Kruskal under the total order (support descending, weight descending, pair index ascending)
  std::vector<int64_t> es;
  for (int64_t k = 0; k < npairs; k++)
    if (!used || used[k]) es.push_back(k);
  std::sort(es.begin(), es.end(), [&](int64_t x, int64_t y) {
    const int32_t sx = support ? support[x] : 0, sy = support ? support[y] : 0;
    if (sx != sy) return sx > sy;
    const double wx = weights ? weights[x] : 1.0, wy = weights ? weights[y] : 1.0;
    if (wx != wy) return wx > wy;
    return x < y;
  });
  std::vector<int> up(nc);
  std::iota(up.begin(), up.end(), 0);
  std::vector<uint8_t> in_tree((size_t)npairs, 0), touched(nc, 0);
  std::vector<double> wsum(nc, 0.0);
  for (int64_t k = 0; k < npairs; k++)  // (in pair order: the sums do not depend on the sort)
    if (!used || used[k]) {
      const size_t a = (size_t)pair_a1[k] - 1, b = (size_t)pair_b1[k] - 1;
      const double w = weights ? weights[k] : 1.0;
      touched[a] = touched[b] = 1;
      wsum[a] += w, wsum[b] += w;
    }
  for (int64_t k : es) {
    const int ra = find_root(up, (int)pair_a1[k] - 1), rb = find_root(up, (int)pair_b1[k] - 1);
    if (ra != rb) up[(size_t)ra] = rb, in_tree[(size_t)k] = 1;
  }
  // components numbered in the order of their lowest camera
  out->component.assign(nc, -1);
  std::vector<int> comp_of_set(nc, -1);
  int ncomp = 0;
  for (size_t c = 0; c < nc; c++)
    if (touched[c]) {
      const int s = find_root(up, (int)c);
      if (comp_of_set[(size_t)s] < 0) comp_of_set[(size_t)s] = ncomp++;
      out->component[c] = comp_of_set[(size_t)s];
    }
  // roots: the lowest fixed camera, else the largest weight sum (ties to the lowest index)
  out->roots.assign((size_t)ncomp, -1);
  std::vector<uint8_t> has_fixed((size_t)ncomp, 0);
  for (size_t c = 0; c < nc; c++) {
    const int g = out->component[c];
    if (g < 0) continue;
    int &r = out->roots[(size_t)g];
    if (fixed && fixed[c]) {
      if (!has_fixed[(size_t)g]) has_fixed[(size_t)g] = 1, r = (int)c;
    } else if (!has_fixed[(size_t)g] && (r < 0 || wsum[c] > wsum[(size_t)r])) {
      r = (int)c;
    }
  }
  // breadth first over the tree edges, the neighbours of a camera in ascending order
  std::vector<int> ptr, nbr, edge;
  view_graph_csr(ncams, npairs, pair_a1, pair_b1, in_tree.data(), &ptr, &nbr, &edge);
  out->parent_pair.assign(nc, -1);
  out->order.clear();
  std::vector<uint8_t> seen(nc, 0);
  for (int g = 0; g < ncomp; g++) {
    size_t head = out->order.size();
    out->order.push_back(out->roots[(size_t)g]);
    seen[(size_t)out->roots[(size_t)g]] = 1;
    for (; head < out->order.size(); head++) {
      const int c = out->order[head];
      for (int e = ptr[(size_t)c]; e < ptr[(size_t)c + 1]; e++) {
        const int j = nbr[(size_t)e];
        if (seen[(size_t)j]) continue;
        seen[(size_t)j] = 1;
        out->parent_pair[(size_t)j] = edge[(size_t)e] >> 1;
        out->order.push_back(j);
      }
    }
  }
}

extern "C" int ba_view_graph_forest(int64_t ncams, int64_t npairs, const int64_t *pair_a1, const int64_t *pair_b1, const uint8_t *used,
                                    const int32_t *support, const double *weights, const uint8_t *fixed, int32_t *component,
                                    int64_t *parent_pair, int64_t *order, int64_t *n_order, int64_t *n_components, int64_t *roots) {
  const char *who = "ba_view_graph_forest";
  if (view_graph_check(who, ncams, npairs, pair_a1, pair_b1)) return BA_ERR_ARG;
  if (!n_order || !n_components || (ncams > 0 && (!component || !parent_pair || !order || !roots))) {
    ba_set_error("%s: null argument", who);
    return BA_ERR_ARG;
  }
  for (int64_t k = 0; weights && k < npairs; k++)
    if (!std::isfinite(weights[k]) || weights[k] < 0) {
      ba_set_error("%s: weights[%lld] = %g: a weight is finite and >= 0", who, (long long)k, weights[k]);
      return BA_ERR_ARG;
    }
  ViewForest f;
  view_graph_forest(ncams, npairs, pair_a1, pair_b1, used, support, weights, fixed, &f);
  for (int64_t c = 0; c < ncams; c++) component[c] = f.component[(size_t)c], parent_pair[c] = f.parent_pair[(size_t)c];
  for (size_t i = 0; i < f.order.size(); i++) order[i] = f.order[i] + 1;
  for (size_t g = 0; g < f.roots.size(); g++) roots[g] = f.roots[g] + 1;
  *n_order = (int64_t)f.order.size();
  *n_components = (int64_t)f.roots.size();
  return BA_OK;
}
