// vk_is_tail.h - the order, the limits, the slices of a chunk and the merge positions of the tail of an importance sample: per
// problem the K largest finite lnpost of the whole sample with their points (vk_is_set_tail / vk_is_tail, include/victor_hip.h;
// victor_amd/importance.py states the definition in NumPy - rule 7 -, DESIGN.md section 7e the kernel mapping).  Header-only and
// free of HIP, like vk_importance.h and vk_is_predict.h: the kernels of vk_kernel_is_tail.h call it, the host side of
// vk_sampled.hip takes its limits and its launch shape from it, and tests/test_importance_tail.py compiles it on its own under
// g++ and drives it the way the kernels do, against np.lexsort.
//
// The order is TOTAL: the larger lnpost first, and between equal values the smaller point index g first.  No two entries share a
// g, so a set of entries has exactly one sorted arrangement, whatever order its members arrived in.
//
// The slices.  A chunk of n rows is cut into gy contiguous blocks of rows, block y the rows block_begin(y) .. block_begin(y + 1)
// - 1, and a block into `per` slices that take its rows in turn: slice (y, sl) holds the rows block_begin(y) + sl + k per.  The
// k-th row of a slice that may enter the tail (a candidate) is written to the slot of the slice's k-th row, so a problem's
// candidate array of n slots needs no counter shared between slices: a slice counts its own, and the slots of two slices never
// meet.  No atomics, and what lies where is the same in every run.
//
// The merge of a sorted held list H (h entries) with a batch C of b candidates sorted by the same order is stated by positions:
//   a held entry e moves to        (its position in H) + (the candidates that precede e)
//   a candidate c goes to          (its position in C) + (the held entries that precede c)
// which is a permutation of 0 .. h + b - 1; the entries whose position is below K are kept.  Both counts are lower bounds of a
// binary search (`preceding`), so a merge costs O((h + b) log) comparisons and no entry is compared with one of its own list.
#pragma once
#include "vk_grid.h"

namespace vkist {

constexpr int kMaxK = 4096;            // entries held per problem: the tail and its cutoff
constexpr int kBlock = 256;            // threads of a workgroup of either kernel
constexpr int kBatch = 1024;           // candidates a merge workgroup sorts in LDS at a time
constexpr int kMaxSlices = 256;        // slices of a chunk: a merge workgroup scans their counts, one per thread
constexpr int kSliceRows = 16;         // rows a slice aims at before the chunk is cut into more blocks
static_assert(kMaxSlices <= kBlock, "one thread per slice count");

// does entry (va, ga) come before entry (vb, gb)?
VK_GRID_HD inline bool precedes(double va, int ga, double vb, int gb) { return va > vb || (va == vb && ga < gb); }

// the entries of a sorted list of n that precede (v, g): at(i, value, index) reads entry i
template <class At>
VK_GRID_HD inline int preceding(int n, double v, int g, At at) {
  int lo = 0, hi = n;                  // entries below lo precede (v, g), entries from hi on do not
  while (lo < hi) {
    const int mid = lo + (hi - lo) / 2;
    double vm;
    int gm;
    at(mid, vm, gm);
    if (precedes(vm, gm, v, g)) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// may a value enter the tail of a problem whose K-th held value is `threshold` (-inf while fewer than K are held)?  A value
// equal to the threshold belongs to a later point than every held entry and stays out; a value that is not finite arrives here
// as -inf (vkgrid::clean) and never enters.
VK_GRID_HD inline bool enters(double v, double threshold) { return v > threshold; }

// problems of a filter workgroup: the power of two >= R, at most 64 (the max kernel's pr) - the problem is the fastest-varying
// lane, so a row of [n][R] coalesces; the workgroup's other kBlock / pr thread groups are the slices of one block of rows
VK_GRID_HD inline int problems_per_block(int R) {
  int pr = 1;
  while (pr < 64 && pr < R) pr *= 2;
  return pr;
}
VK_GRID_HD inline int slices_per_block(int pr) { return kBlock / pr; }
// blocks of rows a chunk of n rows is cut into: slices of about kSliceRows rows, at most kMaxSlices of them
VK_GRID_HD inline int row_blocks(int n, int pr) {
  const int per = slices_per_block(pr), most = kMaxSlices / per;
  const int want = (n + per * kSliceRows - 1) / (per * kSliceRows);
  return want < 1 ? 1 : (want > most ? most : want);
}
VK_GRID_HD inline int block_begin(int n, int gy, int y) { return (int)((long long)n * y / gy); }

// slice s = y per + sl of a chunk: its rows - and the slots of its candidates - are first, first + step, ... below end
struct Slice {
  int first, end, step;
};
VK_GRID_HD inline Slice slice_of(int n, int pr, int gy, int s) {
  const int per = slices_per_block(pr), y = s / per, sl = s - y * per;
  return Slice{block_begin(n, gy, y) + sl, block_begin(n, gy, y + 1), per};
}
VK_GRID_HD inline int rows_of(const Slice& c) { return c.first < c.end ? (c.end - c.first + c.step - 1) / c.step : 0; }

}  // namespace vkist
