// Host-only: the view graph of rotation averaging (ba_view_graph_forest, and the host side of ba_rotation_loops and
// ba_average_rotations; include/ba_hip.h, "rotation averaging").  No HIP in here: ba_view_graph.cpp compiles with
// any C++17 compiler, like ba_order.cpp.
#pragma once
#include <stdint.h>
#include <vector>

// The pairs of an entry: 1-based cameras in 1..ncams, two different cameras, no pair listed twice in either orientation.
// 0, or 1 with `who` in the message of ba_last_error.
int view_graph_check(const char *who, int64_t ncams, int64_t npairs, const int64_t *pair_a1, const int64_t *pair_b1);

// CSR adjacency of the pairs with mask[k] != 0 (null: all): camera c's entries are [ptr[c], ptr[c + 1]), sorted by neighbour;
// nbr = the 0-based neighbour, edge = 2 * pair + orientation (0: c is the pair's first camera, 1: its second)
void view_graph_csr(int64_t ncams, int64_t npairs, const int64_t *pair_a1, const int64_t *pair_b1, const uint8_t *mask,
                    std::vector<int> *ptr, std::vector<int> *nbr, std::vector<int> *edge);

// The maximum spanning forest of ba_view_graph_forest on checked arguments (cameras 0-based in the outputs): component (-1: no
// used pair), parent_pair (-1: root or isolated), order (breadth first from the roots, component after component), roots
struct ViewForest {
  std::vector<int> component, order, roots;
  std::vector<int64_t> parent_pair;
};
void view_graph_forest(int64_t ncams, int64_t npairs, const int64_t *pair_a1, const int64_t *pair_b1, const uint8_t *used,
                       const int32_t *support, const double *weights, const uint8_t *fixed, ViewForest *out);
