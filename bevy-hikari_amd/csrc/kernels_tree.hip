// kernels_tree.hip - tree construction on the device: the Morton-order (LBVH) build, the reference's binned-SAH build (one workgroup,
// and on the whole chip), the forest of mesh trees built at scene load, and the refit of a mesh tree.  Every build ends in the same two
// steps - boxes bottom-up (k_lbvh_boxes), then every node written at its place in every ordering - and writes the `bvh` 0.7.1
// flatten_custom layout the walk expects.  Each construction step exists once, as a device function the single-tree kernel and its
// forest twin both call; the scratch layout of a build is described once (carve_tree_scratch).  Callers: scene_refit.hip
// (hk_rebuild_scene_trees, hk_update_scene_instances), mesh_deform.hip (hk_rebuild_mesh_tree, the refit), scene_load.hip (hk_load_scene).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <utility>
#include <vector>

#include <rocprim/rocprim.hpp>

#include "hk_box.hpp"
#include "hk_device.hpp"
#include "hk_kernels.hpp"

namespace hkd {

// ------------------------------------------------------------------ LBVH rebuild of a flat skip-link BVH (Lauterbach 2009 / Karras 2012)
// hk_rebuild_scene_trees: when motion has degraded a refit tree, a NEW tree over the current leaf boxes is built on the
// device - Morton codes of the box centres, one radix sort (rocPRIM), Karras' parallel hierarchy, boxes bottom-up - and
// written straight into the `bvh` 0.7.1 flatten_custom layout the walk expects: a subtree with L leaves occupies 3L - 2
// consecutive nodes, [navigator of the first child][its subtree][navigator of the second child][its subtree], so the position
// of every node follows from leaf counts alone (no traversal, no stack).  Any binary tree over n shapes has 3n - 2 nodes:
// the new tree fills the old one's storage exactly.  Child order per direction octant = the host's hk_bvh_rethread rule.
struct LbvhBuffers {
  uint32_t n;                   // shapes
  const float4 *box_lo, *box_hi;  // LIGHT: derived from emissives instead
  float* bounds;                // 6 floats: min / max of the box centres (x2)
  uint32_t *codes, *codes_sorted, *ids, *ids_sorted;
  // tree nodes: internal i in [0, n - 1), leaf j as n - 1 + j (j = position in the sorted order)
  uint32_t *parent, *left, *right, *first, *last;  // per internal node (first / last: sorted leaf range it covers)
  uint32_t* leaf_parent;        // per sorted leaf
  float4 *node_lo, *node_hi;    // per tree node (2n - 1)
  uint32_t* arrived;            // per internal node: bottom-up visit counter
  uint8_t* swap;                // per internal node: bit o set = the RIGHT child comes first in ordering o
  uint32_t keep_order0;         // 1: ordering 0 keeps left-before-right (the reference's own flattening of an SAH-built tree)
};
namespace {
__device__ __forceinline__ uint32_t expand_bits(uint32_t v) {  // 10 bits -> every third bit
  v = (v * 0x00010001u) & 0xFF0000FFu;
  v = (v * 0x00000101u) & 0x0F00F00Fu;
  v = (v * 0x00000011u) & 0xC30C30C3u;
  v = (v * 0x00000005u) & 0x49249249u;
  return v;
}
template <bool LIGHT>
__device__ __forceinline__ void lbvh_shape_box(const RefitScene& s, const LbvhBuffers& b, uint32_t shape, f3& mn, f3& mx) {
  if (LIGHT) {
    const float4 pr = s.emissives[shape].position_radius;
    mn = F3(pr.x - pr.w, pr.y - pr.w, pr.z - pr.w);
    mx = F3(pr.x + pr.w, pr.y + pr.w, pr.z + pr.w);
  } else {
    mn = xyz(F4(b.box_lo[shape]));
    mx = xyz(F4(b.box_hi[shape]));
  }
}
// the bounds of the (doubled) box centres of a block's shapes: every thread widens mn / mx by its shapes (centre_bounds_add), the
// block of WAVES waves reduces them and writes min xyz, max xyz to out[0..5]
__device__ __forceinline__ void centre_bounds_add(const f3& lo, const f3& hi, float* mn, float* mx) {
  const float c[3] = {lo.x + hi.x, lo.y + hi.y, lo.z + hi.z};
  for (int k = 0; k < 3; ++k) {
    mn[k] = fminf(mn[k], c[k]);
    mx[k] = fmaxf(mx[k], c[k]);
  }
}
template <int WAVES>
__device__ __forceinline__ void block_centre_bounds(float* mn, float* mx, float* out) {
  __shared__ float red[6][WAVES];
  for (int k = 0; k < 3; ++k)
    for (int off = 32; off > 0; off >>= 1) {
      mn[k] = fminf(mn[k], __shfl_xor(mn[k], off));
      mx[k] = fmaxf(mx[k], __shfl_xor(mx[k], off));
    }
  if ((threadIdx.x & 63u) == 0u)
    for (int k = 0; k < 3; ++k) {
      red[k][threadIdx.x >> 6] = mn[k];
      red[3 + k][threadIdx.x >> 6] = mx[k];
    }
  __syncthreads();
  if (threadIdx.x < 6u) {
    float v = red[threadIdx.x][0];
    for (int w = 1; w < WAVES; ++w) v = threadIdx.x < 3u ? fminf(v, red[threadIdx.x][w]) : fmaxf(v, red[threadIdx.x][w]);
    out[threadIdx.x] = v;
  }
}
// Morton code (30 bits) of a box's centre inside the centre bounds `bounds`
__device__ __forceinline__ uint32_t morton_code(const f3& lo, const f3& hi, const float* bounds) {
  const float c[3] = {lo.x + hi.x, lo.y + hi.y, lo.z + hi.z};
  uint32_t q[3];
  for (int k = 0; k < 3; ++k) {
    const float ext = bounds[3 + k] - bounds[k];
    const float t = ext > 0.0f ? (c[k] - bounds[k]) / ext : 0.0f;
    q[k] = (uint32_t)fminf(fmaxf(t * 1024.0f, 0.0f), 1023.0f);
  }
  return (expand_bits(q[0]) << 2) | (expand_bits(q[1]) << 1) | expand_bits(q[2]);
}
// common prefix length of the (code, position) keys of sorted leaves i and j; -1 outside the array
__device__ __forceinline__ int lbvh_delta(const uint32_t* __restrict__ codes, int n, int i, int j) {
  if (j < 0 || j >= n) return -1;
  const uint32_t a = codes[i], c = codes[j];
  if (a != c) return __clz((int)(a ^ c));
  return 32 + __clz(i ^ j);
}
// Karras 2012, "Maximizing Parallelism in the Construction of BVHs, Octrees, and k-d Trees", section 4: internal node i of the tree over
// the n sorted codes at b.codes_sorted + base, whose internal node k is tree node base + k and whose leaf j is tree node b.n - 1 + base + j
// (a single tree: base 0) - its children, the leaf range it covers, its children's parent links
__device__ __forceinline__ void karras_node(const LbvhBuffers& b, uint32_t base, int n, int i) {
  const uint32_t* codes = b.codes_sorted + base;
  const int d = (lbvh_delta(codes, n, i, i + 1) - lbvh_delta(codes, n, i, i - 1)) >= 0 ? 1 : -1;
  const int dmin = lbvh_delta(codes, n, i, i - d);
  int lmax = 2;
  while (lbvh_delta(codes, n, i, i + lmax * d) > dmin) lmax <<= 1;
  int l = 0;
  for (int t = lmax >> 1; t >= 1; t >>= 1)
    if (lbvh_delta(codes, n, i, i + (l + t) * d) > dmin) l += t;
  const int j = i + l * d;
  const int dnode = lbvh_delta(codes, n, i, j);
  int sft = 0;
  for (int t = (l + 1) >> 1;; t = (t + 1) >> 1) {
    if (lbvh_delta(codes, n, i, i + (sft + t) * d) > dnode) sft += t;
    if (t <= 1) break;
  }
  const int gamma = i + sft * d + min(d, 0);
  const int lo = min(i, j), hi = max(i, j);
  const uint32_t g = base + (uint32_t)i, leaf0 = b.n - 1u + base;
  const bool l_leaf = lo == gamma, r_leaf = hi == gamma + 1;
  const uint32_t lc = l_leaf ? leaf0 + (uint32_t)gamma : base + (uint32_t)gamma;  // leaf gamma or internal gamma
  const uint32_t rc = r_leaf ? leaf0 + (uint32_t)gamma + 1u : base + (uint32_t)gamma + 1u;
  b.left[g] = lc;
  b.right[g] = rc;
  b.first[g] = base + (uint32_t)lo;
  b.last[g] = base + (uint32_t)hi;
  if (l_leaf) b.leaf_parent[base + (uint32_t)gamma] = g; else b.parent[lc] = g;
  if (r_leaf) b.leaf_parent[base + (uint32_t)gamma + 1u] = g; else b.parent[rc] = g;
  if (i == 0) b.parent[g] = HK_U32_MAX;
}
// Tree node v (parent p) of a tree of `leaves` shapes into ordering o of the tree's node array (nlo / nhi = its node 0, `stride` float4
// between nodes): every node except the root writes the navigator in front of its subtree; a leaf (of `shape`) also writes its own slot.
// The start of the subtree: walk to the root (whose parent is HK_U32_MAX); a first child starts one node after its parent's start (its
// navigator), a second child after the whole first branch.  FOREST: the arrays hold many trees and ids no tree uses, so the walk ends at
// anything that is no internal node and nothing is written outside the tree's 3 * leaves - 2 nodes, whatever the arrays hold; a single
// tree's caller passes no root.
template <bool FOREST>
__device__ __forceinline__ void emit_tree_node(const LbvhBuffers& b, uint32_t v, uint32_t p, uint32_t o, uint32_t shape, uint32_t leaves, float4* nlo, float4* nhi,
                                               uint32_t stride) {
  const uint32_t n = b.n;
  const bool leaf = v >= n - 1u;
  const float4 blo = b.node_lo[v], bhi = b.node_hi[v];
  if (leaves == 1u) {  // flatten_custom of a single leaf: the leaf alone
    nlo[0] = make_float4(blo.x, blo.y, blo.z, u2f(HK_LEAF | shape));
    nhi[0] = make_float4(bhi.x, bhi.y, bhi.z, u2f(1u));
    return;
  }
  auto leaves_of = [&](uint32_t node) { return node >= n - 1u ? 1u : b.last[node] - b.first[node] + 1u; };
  uint32_t start = 0u, c = v;
  while (FOREST ? p < n - 1u : p != HK_U32_MAX) {
    const bool right_first = (b.swap[p] >> o) & 1u;
    const uint32_t first_child = right_first ? b.right[p] : b.left[p];
    start += (c == first_child) ? 1u : 2u + (3u * leaves_of(first_child) - 2u);
    c = p;
    p = b.parent[p];
  }
  const uint32_t size = 3u * leaves_of(v) - 2u;
  if (FOREST && (start == 0u || start > 3u * leaves - 2u - size)) return;
  // the navigator: entry = its subtree, exit = past it; a leaf's is folded (scene_layout.hip fold_leaf_navigators) - it is the leaf slot over again
  const float4 nav_lo = make_float4(blo.x, blo.y, blo.z, u2f(leaf ? HK_LEAF | shape : start));
  const float4 nav_hi = make_float4(bhi.x, bhi.y, bhi.z, u2f(leaf ? start + 1u : start + size));
  nlo[(size_t)(start - 1u) * stride] = nav_lo;
  nhi[(size_t)(start - 1u) * stride] = nav_hi;
  if (leaf) {
    nlo[(size_t)start * stride] = nav_lo;
    nhi[(size_t)start * stride] = nav_hi;
  }
}
}  // namespace

template <bool LIGHT>
__global__ __launch_bounds__(1024) void k_lbvh_bounds(RefitScene s, LbvhBuffers b) {  // one workgroup
  float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (uint32_t i = threadIdx.x; i < b.n; i += 1024u) {
    f3 lo, hi;
    lbvh_shape_box<LIGHT>(s, b, i, lo, hi);
    centre_bounds_add(lo, hi, mn, mx);
  }
  block_centre_bounds<16>(mn, mx, b.bounds);
}
template <bool LIGHT>
__global__ __launch_bounds__(256) void k_lbvh_codes(RefitScene s, LbvhBuffers b) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= b.n) return;
  f3 lo, hi;
  lbvh_shape_box<LIGHT>(s, b, i, lo, hi);
  b.codes[i] = morton_code(lo, hi, b.bounds);
  b.ids[i] = i;
}
// one thread per internal node
__global__ __launch_bounds__(256) void k_lbvh_hierarchy(LbvhBuffers b) {
  const int n = (int)b.n, i = (int)(blockIdx.x * 256u + threadIdx.x);
  if (i >= n - 1) return;
  karras_node(b, 0u, n, i);
}
// leaf boxes, then every internal node by the second of its children to arrive (min / max are exact: any order gives the same box)
template <bool LIGHT>
__device__ __forceinline__ void lbvh_leaf_climb(const RefitScene& s, const LbvhBuffers& b, uint32_t j) {
  f3 mn, mx;
  lbvh_shape_box<LIGHT>(s, b, b.ids_sorted[j], mn, mx);
  b.node_lo[b.n - 1u + j] = make_float4(mn.x, mn.y, mn.z, 0.0f);
  b.node_hi[b.n - 1u + j] = make_float4(mx.x, mx.y, mx.z, 0.0f);
  if (b.n == 1u) return;
  uint32_t p = b.leaf_parent[j];
  if (p == HK_U32_MAX) return;  // (a forest build: the only leaf of a one-triangle tree)
  for (;;) {
    __threadfence();
    if (atomicAdd(&b.arrived[p], 1u) == 0u) return;  // the sibling subtree is not finished: its thread continues from here
    __threadfence();
    const uint32_t l = b.left[p], r = b.right[p];
    const volatile float4* vlo = b.node_lo;
    const volatile float4* vhi = b.node_hi;
    const f3 al = F3(vlo[l].x, vlo[l].y, vlo[l].z), ah = F3(vhi[l].x, vhi[l].y, vhi[l].z);
    const f3 bl = F3(vlo[r].x, vlo[r].y, vlo[r].z), bh = F3(vhi[r].x, vhi[r].y, vhi[r].z);
    b.node_lo[p] = make_float4(hmin(al.x, bl.x), hmin(al.y, bl.y), hmin(al.z, bl.z), 0.0f);
    b.node_hi[p] = make_float4(hmax(ah.x, bh.x), hmax(ah.y, bh.y), hmax(ah.z, bh.z), 0.0f);
    // child order per direction octant: host_logic.cpp rethread_flat_bvh (the axis along which the two boxes are furthest apart)
    int axis = 0;
    float best = -1.0f, ca_axis = 0.0f, cb_axis = 0.0f;
    const float ca[3] = {al.x + ah.x, al.y + ah.y, al.z + ah.z}, cb[3] = {bl.x + bh.x, bl.y + bh.y, bl.z + bh.z};
    for (int k = 0; k < 3; ++k) {
      const float dd = fabsf(ca[k] - cb[k]);
      if (dd > best) { best = dd; axis = k; ca_axis = ca[k]; cb_axis = cb[k]; }
    }
    const bool a_lower = ca_axis <= cb_axis;
    uint32_t sw = 0u;
    for (uint32_t o = 0; o < 8u; ++o) {
      const bool negative = (o >> axis) & 1u;
      if (!(a_lower != negative)) sw |= 1u << o;
    }
    if (b.keep_order0) sw &= ~1u;
    b.swap[p] = (uint8_t)sw;
    p = b.parent[p];
    if (p == HK_U32_MAX) return;
  }
}
template <bool LIGHT>
__global__ __launch_bounds__(256) void k_lbvh_boxes(RefitScene s, LbvhBuffers b) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= b.n) return;
  lbvh_leaf_climb<LIGHT>(s, b, j);
}
// thread t of (tree nodes x orderings) of a single tree: its node into its ordering (emit_tree_node)
__device__ __forceinline__ void lbvh_emit_node(const LbvhBuffers& b, uint32_t t, float4* lo, float4* hi, uint32_t stride, size_t ord_stride, uint32_t orderings) {
  const uint32_t n = b.n, total = 2u * n - 1u;
  if (t >= total * orderings) return;
  const uint32_t o = t / total, v = t - o * total;
  const bool leaf = v >= n - 1u;
  const uint32_t shape = leaf ? b.ids_sorted[v - (n - 1u)] : 0u;
  if (n > 1u && v == 0u) return;  // the root has no navigator
  const uint32_t p = n == 1u ? HK_U32_MAX : leaf ? b.leaf_parent[v - (n - 1u)] : b.parent[v];  // (n == 1: the leaf alone)
  emit_tree_node<false>(b, v, p, o, shape, n, lo + (size_t)o * ord_stride, hi + (size_t)o * ord_stride, stride);
}
// one thread per tree node and ordering
__global__ __launch_bounds__(256) void k_lbvh_emit(LbvhBuffers b, float4* lo, float4* hi, uint32_t stride, size_t ord_stride /* float4 between orderings */, uint32_t orderings) {
  lbvh_emit_node(b, blockIdx.x * 256u + threadIdx.x, lo, hi, stride, ord_stride, orderings);
}
// the buffers of a REFIT of a mesh tree: its fixed topology, leaf boxes = the triangle boxes, ordering 0 kept left before right
__host__ __device__ inline LbvhBuffers mesh_refit_buffers(const MeshTree& t) {
  LbvhBuffers b{};
  b.n = t.n;
  b.box_lo = t.tri_lo; b.box_hi = t.tri_hi;
  b.ids_sorted = t.leaf_shape;
  b.parent = t.parent; b.left = t.left; b.right = t.right; b.first = t.first; b.last = t.last; b.leaf_parent = t.leaf_parent;
  b.node_lo = t.node_lo; b.node_hi = t.node_hi; b.arrived = t.arrived; b.swap = t.swap;
  b.keep_order0 = 1u;
  return b;
}
// the refit of the trees of many meshes (hk_deform_meshes): k_lbvh_boxes and k_lbvh_emit, every workgroup on 256 leaves / (node, ordering)
// pairs of ONE item's tree (hk_kernels.hpp SegmentBlock), each tree into its own node range of every ordering.  The arrival counters
// were zeroed by kernels_deform.hip k_deform_triangles.
__global__ __launch_bounds__(256) void k_deform_boxes(const DeformItem* __restrict__ items, const SegmentBlock* __restrict__ blocks) {
  const SegmentBlock bl = blocks[blockIdx.x];
  const LbvhBuffers b = mesh_refit_buffers(items[bl.segment].tree);
  const uint32_t j = bl.first + threadIdx.x;
  if (j >= b.n) return;
  const RefitScene none{};
  lbvh_leaf_climb<false>(none, b, j);
}
__global__ __launch_bounds__(256) void k_deform_emit(const DeformItem* __restrict__ items, const SegmentBlock* __restrict__ blocks, size_t ord_stride, uint32_t orderings) {
  const SegmentBlock bl = blocks[blockIdx.x];
  const DeformItem* it = items + bl.segment;
  const LbvhBuffers b = mesh_refit_buffers(it->tree);
  float4* lo = it->nodes;
  lbvh_emit_node(b, bl.first + threadIdx.x, lo, lo + 1, 2u, ord_stride, orderings);
}


// ------------------------------------------------------------------ the reference's own tree, built on the device
// `bvh` 0.7.1 BVHNode::build (scene_builder.cpp build_recursive; the crate the reference calls at instance.rs:365-371,422-428) is a
// top-down binned SAH: per node the bounds of the shapes and of their centres, the longest axis of the centre bounds, six buckets
// along it, the cheapest of the five splits, the shapes re-ordered bucket by bucket.  Every reduction in it is a min, a max or a
// count, and the re-ordering is a STABLE sort by bucket: nothing depends on the order in which a parallel machine visits the
// shapes.  So the same tree can be built level by level: one workgroup, all nodes of a level at once, the shapes in one array
// that is stably re-sorted per level (block scans of the six bucket flags, segmented at node boundaries, with running counters
// per node and bucket across the 1024-item chunks).  The costs are the host's float expressions term for term, so the splits -
// and with them the shape of the tree - are the host's: tests compare the entry / exit links with the host builder's arrays.
// (Zeros may come out with the other sign than std::min / std::max chains give - a box bound of -0 vs +0 changes no decision.)
struct SahBuffers {
  uint32_t* order[2];      // shape ids, segment by segment
  uint32_t* item_node[2];  // per position: the internal node whose segment it is in, or SAH_DONE once it is a leaf
  uint8_t* item_bucket;
  uint32_t* active[2];     // internal nodes split at this level / created for the next
  uint32_t* acc;           // per internal node: 54 words - bounds (6), centre bounds (6), 6 bucket boxes (36), 6 bucket counts
  float* split;            // per internal node: 4 words - centre-bounds min on the axis, axis size, (bits) axis, (bits) half-split flag
  uint32_t* offsets;       // per internal node: 14 words - first target position of each bucket (6), running counts (6), left count, split bucket
  uint32_t* node_level;    // per internal node: the level of the loop that splits it
  uint32_t* roots;         // nodes handed to k_sah_subtrees
  uint32_t* counters;      // [0] internal nodes allocated, [1] subtree roots, [2] the ping-pong side the top of the tree ended on
};
namespace {
constexpr uint32_t SAH_DONE = 0xFFFFFFFFu;
__device__ __forceinline__ float box_center(float mn, float mx) { return mn + (mx - mn) / 2.0f; }  // Box::center
__device__ __forceinline__ float box_area(const float* mn, const float* mx) {                      // Box::surface_area
  const float x = mx[0] - mn[0], y = mx[1] - mn[1], z = mx[2] - mn[2];
  return 2.0f * (x * y + x * z + y * z);
}
// word w of a node's accumulators when nothing has been added: an empty box (min xyz, max xyz) below word 48, a count of 0 from there
__device__ __forceinline__ uint32_t sah_acc_init(uint32_t w) { return w < 48u ? ((w % 6u) < 3u ? box_word(INFINITY) : box_word(-INFINITY)) : 0u; }
// is `node` (of an item: SAH_DONE = a leaf already) split at `level`
__device__ __forceinline__ bool sah_splitting(const SahBuffers& q, uint32_t node, uint32_t level) { return node != SAH_DONE && q.node_level[node] == level; }
// min / max of a box into the accumulator words acc[0..5] (keys): when every lane of the wave that takes part adds to the SAME
// accumulator (the top levels of the tree: thousands of shapes per node) the wave reduces first - one hot address takes ~10 ns per
// atomic - otherwise every lane adds on its own.  Called by all lanes of the wave; `take` = this lane has a box for `acc`.
__device__ __forceinline__ void wave_box_accumulate(uint32_t* acc, bool take, const float* mn, const float* mx, uint32_t* count) {
  const unsigned long long m = __ballot(take);
  if (m == 0ull) return;
  const unsigned long long a = (unsigned long long)(size_t)acc;
  const int leader = __ffsll((long long)m) - 1;
  const unsigned long long a0 = __shfl(a, leader);
  const bool uniform = __ballot(take && a != a0) == 0ull;
  if (uniform) {
    float lo[3], hi[3];
    for (int k = 0; k < 3; ++k) {
      lo[k] = take ? mn[k] : INFINITY;
      hi[k] = take ? mx[k] : -INFINITY;
      for (int off = 32; off > 0; off >>= 1) {
        lo[k] = fminf(lo[k], __shfl_xor(lo[k], off));
        hi[k] = fmaxf(hi[k], __shfl_xor(hi[k], off));
      }
    }
    if ((int)(threadIdx.x & 63u) == leader) {
      for (int k = 0; k < 3; ++k) {
        atomicMin(&acc[k], box_word(lo[k]));
        atomicMax(&acc[3 + k], box_word(hi[k]));
      }
      if (count) atomicAdd(count, (uint32_t)__popcll(m));
    }
  } else if (take) {
    for (int k = 0; k < 3; ++k) {
      atomicMin(&acc[k], box_word(mn[k]));
      atomicMax(&acc[3 + k], box_word(mx[k]));
    }
    if (count) atomicAdd(count, 1u);
  }
}
// the six bucket-flag prefix sums (packed two 16-bit counters per word: a chunk has 1024 items) and the run-head maximum of a chunk
// in ONE pass: three block barriers instead of twenty-one.  lds: 4 x 17 words
__device__ __forceinline__ void block_scan_buckets_and_heads(uint32_t bk, uint32_t head_value, uint32_t* lds, uint32_t pre[3], uint32_t& head) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t v[3] = {0u, 0u, 0u};
  if (bk < 6u) v[bk >> 1] = 1u << (16u * (bk & 1u));
  uint32_t inc[3] = {v[0], v[1], v[2]}, hmax = head_value;
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t t0 = __shfl_up(inc[0], off), t1 = __shfl_up(inc[1], off), t2 = __shfl_up(inc[2], off), th = __shfl_up(hmax, off);
    if ((int)lane >= off) {
      inc[0] += t0;
      inc[1] += t1;
      inc[2] += t2;
      hmax = max(hmax, th);
    }
  }
  __syncthreads();
  if (lane == 63u) {
    lds[wave] = inc[0];
    lds[17 + wave] = inc[1];
    lds[34 + wave] = inc[2];
    lds[51 + wave] = hmax;
  }
  __syncthreads();
  if (threadIdx.x < 4u) {
    uint32_t* a = lds + 17u * threadIdx.x;
    uint32_t run = 0u;
    for (int w = 0; w < 16; ++w) {
      const uint32_t t = a[w];
      a[w] = run;
      run = threadIdx.x == 3u ? max(run, t) : run + t;
    }
  }
  __syncthreads();
  for (int k = 0; k < 3; ++k) pre[k] = lds[17 * k + wave] + inc[k] - v[k];
  head = max(lds[51 + wave], hmax);
}

// ---- the steps of a level, per item (a position of the shape array) or per node: sah_levels runs them inside one workgroup, k_sahw_*
// one launch each over the whole chip.  Steps with wave reductions are called by whole waves; `take` = this lane's item takes part.
template <bool LIGHT>
__device__ __forceinline__ void sah_item_box(const RefitScene& s, const LbvhBuffers& b, uint32_t shape, float* mn, float* mx) {
  f3 lo, hi;
  lbvh_shape_box<LIGHT>(s, b, shape, lo, hi);
  mn[0] = lo.x; mn[1] = lo.y; mn[2] = lo.z;
  mx[0] = hi.x; mx[1] = hi.y; mx[2] = hi.z;
}
// step B, per item: the box of the shape at position p into the bounds (acc[0..5]) and the centre bounds (acc[6..11])
template <bool LIGHT>
__device__ __forceinline__ void sah_item_bounds(const RefitScene& s, const LbvhBuffers& b, uint32_t* acc, bool take, const uint32_t* order, uint32_t p) {
  float mn[3] = {0, 0, 0}, mx[3] = {0, 0, 0}, cc[3] = {0, 0, 0};
  if (take) {
    sah_item_box<LIGHT>(s, b, order[p], mn, mx);
    for (int k = 0; k < 3; ++k) cc[k] = box_center(mn[k], mx[k]);
  }
  wave_box_accumulate(acc, take, mn, mx, nullptr);
  wave_box_accumulate(acc + 6, take, cc, cc, nullptr);
}
// step C, per node: the split axis from its centre bounds (Box::largest_axis), and whether its shapes are too close together
__device__ __forceinline__ void sah_split_axis(const SahBuffers& q, uint32_t node) {
  const uint32_t* acc = q.acc + (size_t)node * 54u;
  float cmn[3], cmx[3];
  for (int k = 0; k < 3; ++k) {
    cmn[k] = box_unword(acc[6 + k]);
    cmx[k] = box_unword(acc[9 + k]);
  }
  const float x = cmx[0] - cmn[0], y = cmx[1] - cmn[1], z = cmx[2] - cmn[2];
  const int axis = (x > y && x > z) ? 0 : (y > z ? 1 : 2);  // Box::largest_axis
  const float axis_size = cmx[axis] - cmn[axis];
  float* sp = q.split + (size_t)node * 4u;
  sp[0] = cmn[axis];
  sp[1] = axis_size;
  sp[2] = u2f((uint32_t)axis);
  sp[3] = u2f(axis_size < 0.00001f ? 1u : 0u);  // shapes too close together: the index list is cut in half
}
// step D, per item at position p of a node split at this level (`take`; cleared where the node takes the half cut): its box and its
// bucket along the node's axis, which is returned and left in item_bucket[p]
template <bool LIGHT>
__device__ __forceinline__ int sah_item_bucket(const RefitScene& s, const LbvhBuffers& b, const SahBuffers& q, uint32_t node, const uint32_t* order, uint32_t p, bool& take,
                                               float* mn, float* mx) {
  int bk = 0;
  if (take) {
    const float* sp = q.split + (size_t)node * 4u;
    take = f2u(sp[3]) == 0u;
    if (take) {
      sah_item_box<LIGHT>(s, b, order[p], mn, mx);
      const int axis = (int)f2u(sp[2]);
      const float rel = (box_center(mn[axis], mx[axis]) - sp[0]) / sp[1];
      bk = (int)(rel * (6.0f - 0.01f));
      bk = min(max(bk, 0), 5);
      q.item_bucket[p] = (uint8_t)bk;
    }
  }
  return bk;
}
// step E, per node: the cheapest of the five splits (the host's float expressions term for term), its bucket offsets and its
// children - `child` receives their tree nodes.  A child to split at the next level is appended to active_out[*n_out]
__device__ __forceinline__ void sah_split_node(const LbvhBuffers& b, const SahBuffers& q, uint32_t node, uint32_t level, uint32_t defer, uint32_t* active_out,
                                               uint32_t* n_out, uint32_t child[2]) {
  const uint32_t n = b.n;
  const uint32_t* acc = q.acc + (size_t)node * 54u;
  const float* sp = q.split + (size_t)node * 4u;
  uint32_t* off = q.offsets + (size_t)node * 14u;
  const uint32_t begin = b.first[node], count = b.last[node] - begin + 1u;
  uint32_t n_left = count / 2u, split_bucket = 6u;  // 6: cut the list in half
  if (f2u(sp[3]) == 0u) {
    float bounds_mn[3], bounds_mx[3];
    for (int k = 0; k < 3; ++k) {
      bounds_mn[k] = box_unword(acc[k]);
      bounds_mx[k] = box_unword(acc[3 + k]);
    }
    const float total_area = box_area(bounds_mn, bounds_mx);
    float min_cost = INFINITY;
    uint32_t min_bucket = 0u;
    for (uint32_t i = 0; i < 5u; ++i) {
      float lmn[3] = {INFINITY, INFINITY, INFINITY}, lmx[3] = {-INFINITY, -INFINITY, -INFINITY};
      float rmn[3] = {INFINITY, INFINITY, INFINITY}, rmx[3] = {-INFINITY, -INFINITY, -INFINITY};
      uint32_t ln = 0u, rn = 0u;
      for (uint32_t k6 = 0; k6 < 6u; ++k6) {
        const uint32_t* bb = acc + 12u + 6u * k6;
        float* tmn = k6 <= i ? lmn : rmn;
        float* tmx = k6 <= i ? lmx : rmx;
        for (int k = 0; k < 3; ++k) {
          tmn[k] = hmin(tmn[k], box_unword(bb[k]));
          tmx[k] = hmax(tmx[k], box_unword(bb[3 + k]));
        }
        if (k6 <= i) ln += acc[48u + k6]; else rn += acc[48u + k6];
      }
      const float cost = ((float)ln * box_area(lmn, lmx) + (float)rn * box_area(rmn, rmx)) / total_area;
      if (cost < min_cost) {
        min_bucket = i;
        min_cost = cost;
      }
    }
    uint32_t best_left = 0u;  // (all costs NaN: the host keeps bucket 0 as the split)
    for (uint32_t k6 = 0; k6 <= min_bucket; ++k6) best_left += acc[48u + k6];
    if (best_left != 0u && best_left != count) {
      n_left = best_left;
      split_bucket = min_bucket;
    }  // (an empty side - NaN costs - falls back to the half cut, like the host)
  }
  uint32_t run = begin;
  for (uint32_t k6 = 0; k6 < 6u; ++k6) {
    off[k6] = run;
    run += acc[48u + k6];
    off[6u + k6] = 0u;
  }
  off[12] = n_left;
  off[13] = split_bucket;
  // children: a side with one shape is a leaf at its position, a larger one an internal node - split at the next level, or
  // handed to a workgroup of its own when it is small enough
  const uint32_t n_right = count - n_left;
  for (int side = 0; side < 2; ++side) {
    const uint32_t c_begin = side == 0 ? begin : begin + n_left, c_count = side == 0 ? n_left : n_right;
    if (c_count == 1u) {
      child[side] = (n - 1u) + c_begin;
      b.leaf_parent[c_begin] = node;
    } else {
      const uint32_t id = atomicAdd(&q.counters[0], 1u);
      child[side] = id;
      b.first[id] = c_begin;
      b.last[id] = c_begin + c_count - 1u;
      b.parent[id] = node;
      if (c_count <= defer) {
        q.node_level[id] = SAH_DONE;  // (not a level of this loop)
        q.roots[atomicAdd(&q.counters[1], 1u)] = id;
      } else {
        q.node_level[id] = level + 1u;
        active_out[atomicAdd(n_out, 1u)] = id;
      }
    }
  }
  b.left[node] = child[0];
  b.right[node] = child[1];
}
// step F, the stable re-order bucket by bucket inside every segment, over one chunk of 1024 positions from c0 of the range that ends
// at r1.  What an item is to the re-order of `level`:
struct SahItem {
  uint32_t node;   // the node whose segment it is in, SAH_DONE: a leaf already (or past the end)
  uint32_t bk;     // its bucket, 7: it does not move (its node is not split now, or takes the half cut)
  bool in, split_now, moving;
};
// ... with the exclusive prefix of every bucket's flags inside the chunk left in pre[][tid]; returns the position in the chunk at
// which the item's run (the items of its node) begins
__device__ __forceinline__ uint32_t sah_reorder_scan(const SahBuffers& q, const uint32_t* item_node, uint32_t c0, uint32_t r1, uint32_t level, uint32_t* scan_lds,
                                                     uint16_t (*pre)[1024], SahItem& it) {
  const uint32_t tid = threadIdx.x, p = c0 + tid;
  it.in = p < r1;
  it.node = it.in ? item_node[p] : SAH_DONE;
  it.split_now = it.in && sah_splitting(q, it.node, level);
  it.moving = it.split_now && q.offsets[(size_t)it.node * 14u + 13u] != 6u;
  it.bk = it.moving ? q.item_bucket[p] : 7u;
  const bool head = tid == 0u || !it.in || item_node[p - 1u] != it.node;
  uint32_t packed[3], h;
  block_scan_buckets_and_heads(it.bk, head ? tid : 0u, scan_lds, packed, h);
  for (uint32_t k6 = 0; k6 < 6u; ++k6) pre[k6][tid] = (uint16_t)((packed[k6 >> 1] >> (16u * (k6 & 1u))) & 0xFFFFu);
  return h;
}
// ... and the item at position p written to its place on the other side.  A moving item goes behind the items of its node and bucket
// before it: those of its run in this chunk (pre, from the run's head h) and those of earlier chunks, which carried() counts (called for
// a moving item only).  A leaf already, or an item of a node that waits for a workgroup of its own, keeps its place
template <typename Carried>
__device__ __forceinline__ void sah_reorder_place(const LbvhBuffers& b, const SahBuffers& q, const SahItem& it, uint32_t p, uint32_t h, const uint16_t (*pre)[1024],
                                                  Carried carried, const uint32_t* order, uint32_t* order_out, uint32_t* item_node_out) {
  if (it.split_now) {
    const uint32_t* off = q.offsets + (size_t)it.node * 14u;
    const uint32_t begin = b.first[it.node], n_left = off[12];
    uint32_t target = p;
    if (it.moving) target = off[it.bk] + carried() + ((uint32_t)pre[it.bk][threadIdx.x] - (uint32_t)pre[it.bk][h]);
    const bool goes_left = target < begin + n_left;
    const uint32_t child = goes_left ? b.left[it.node] : b.right[it.node];
    order_out[target] = order[p];
    item_node_out[target] = child >= b.n - 1u ? SAH_DONE : child;
  } else if (it.in) {
    order_out[p] = order[p];
    item_node_out[p] = it.node;
  }
}
}  // namespace

// The level loop over one range [r0, r1) of item positions, run by ONE workgroup of 1024 threads: every node of a level at once.
// `first_level`: node_level value of the range's root (the nodes created below get first_level + 1, ...).  Nodes with at most
// `defer` shapes are not split here but appended to q.roots (their subtrees are built by k_sah_subtrees, one workgroup each, all
// at once).  Returns the ping-pong side that holds the range's final order.
template <bool LIGHT>
__device__ uint32_t sah_levels(const RefitScene& s, const LbvhBuffers& b, const SahBuffers& q, uint32_t r0, uint32_t r1, uint32_t root, uint32_t cur, uint32_t first_level,
                               uint32_t defer) {
  __shared__ uint32_t scan_lds[68];
  __shared__ uint16_t pre[6][1024];  // per chunk: exclusive prefix of each bucket's flags
  __shared__ uint32_t head_of[1024];
  __shared__ uint32_t n_active_lds[2];
  const uint32_t tid = threadIdx.x;
  if (tid == 0u) {
    q.active[cur][r0] = root;
    q.node_level[root] = first_level;
    n_active_lds[cur] = 1u;
    n_active_lds[cur ^ 1u] = 0u;
  }
  __syncthreads();
  for (uint32_t level = first_level;; ++level) {  // (a level with nothing to split ends the loop)
    const uint32_t n_active = n_active_lds[cur];
    if (n_active == 0u) break;
    const uint32_t* order = q.order[cur];
    const uint32_t* item_node = q.item_node[cur];
    uint32_t* order_out = q.order[cur ^ 1u];
    uint32_t* item_node_out = q.item_node[cur ^ 1u];
    const uint32_t* active = q.active[cur] + r0;
    uint32_t* active_out = q.active[cur ^ 1u] + r0;
    // A: accumulators
    for (uint32_t a = tid; a < n_active * 54u; a += 1024u) q.acc[(size_t)active[a / 54u] * 54u + a % 54u] = sah_acc_init(a % 54u);
    __syncthreads();
    if (tid == 0u) n_active_lds[cur ^ 1u] = 0u;
    // B: bounds of the shapes and of their centres
    for (uint32_t p0 = r0; p0 < r1; p0 += 1024u) {  // (block-uniform trip count: the wave reductions want whole waves)
      const uint32_t p = p0 + tid;
      const uint32_t node = p < r1 ? item_node[p] : SAH_DONE;
      const bool take = sah_splitting(q, node, level);
      sah_item_bounds<LIGHT>(s, b, q.acc + (size_t)(take ? node : 0u) * 54u, take, order, p);
    }
    __syncthreads();
    // C: split axis
    for (uint32_t a = tid; a < n_active; a += 1024u) sah_split_axis(q, active[a]);
    __syncthreads();
    // D: buckets
    for (uint32_t p0 = r0; p0 < r1; p0 += 1024u) {
      const uint32_t p = p0 + tid;
      const uint32_t node = p < r1 ? item_node[p] : SAH_DONE;
      bool take = sah_splitting(q, node, level);
      float mn[3] = {0, 0, 0}, mx[3] = {0, 0, 0};
      const int bk = sah_item_bucket<LIGHT>(s, b, q, node, order, p, take, mn, mx);
      for (int k6 = 0; k6 < 6; ++k6) {  // bucket by bucket: lanes of one node and one bucket share an accumulator
        const bool mine = take && bk == k6;
        uint32_t* acc = q.acc + (size_t)(mine ? node : 0u) * 54u;
        wave_box_accumulate(acc + 12 + 6 * k6, mine, mn, mx, acc + 48 + k6);
      }
    }
    __syncthreads();
    // E: the cheapest split, the children
    for (uint32_t a = tid; a < n_active; a += 1024u) {
      uint32_t child[2];
      sah_split_node(b, q, active[a], level, defer, active_out, &n_active_lds[cur ^ 1u], child);
    }
    __syncthreads();
    // F: chunk after chunk, so that the running counts (offsets[6..11] of the node) stay in order
    for (uint32_t c0 = r0; c0 < r1; c0 += 1024u) {
      const uint32_t p = c0 + tid;
      SahItem it;
      const uint32_t h = sah_reorder_scan(q, item_node, c0, r1, level, scan_lds, pre, it);
      head_of[tid] = h;
      __syncthreads();
      auto carried = [&]() { return q.offsets[(size_t)it.node * 14u + 6u + it.bk]; };  // (the node's running count)
      sah_reorder_place(b, q, it, p, h, pre, carried, order, order_out, item_node_out);
      __syncthreads();
      // the last item of a node's run in this chunk adds the chunk's counts to the node's running counts
      if (it.moving) {
        const bool last_of_run = tid == 1023u || p + 1u >= r1 || item_node[p + 1u] != it.node;
        if (last_of_run) {
          uint32_t* off = q.offsets + (size_t)it.node * 14u;
          for (uint32_t k6 = 0; k6 < 6u; ++k6) off[6u + k6] += ((uint32_t)pre[k6][tid] + (it.bk == k6 ? 1u : 0u)) - (uint32_t)pre[k6][h];
        }
      }
      __syncthreads();
    }
    cur ^= 1u;
  }
  __syncthreads();
  return cur;
}

// SAH_SUBTREE: nodes with at most this many shapes are built by a workgroup of their own (k_sah_subtrees), all of them at once
constexpr uint32_t SAH_SUBTREE = 1024u;
// the top of the tree: one workgroup over the whole array, down to nodes of at most SAH_SUBTREE shapes.  Outputs the LbvhBuffers
// topology (ids_sorted = leaf order, parent / left / right / first / last / leaf_parent) for k_lbvh_boxes + k_lbvh_emit
template <bool LIGHT>
__global__ __launch_bounds__(1024) void k_sah_build(RefitScene s, LbvhBuffers b, SahBuffers q) {
  const uint32_t n = b.n, tid = threadIdx.x;
  if (n == 1u) {
    if (tid == 0u) {
      b.ids_sorted[0] = 0u;
      q.counters[1] = 0u;
    }
    return;
  }
  for (uint32_t i = tid; i < n; i += 1024u) {
    q.order[0][i] = i;
    q.item_node[0][i] = 0u;
  }
  if (tid == 0u) {
    b.first[0] = 0u;
    b.last[0] = n - 1u;
    b.parent[0] = HK_U32_MAX;
    q.counters[0] = 1u;  // internal nodes allocated
    q.counters[1] = 0u;  // subtree roots
  }
  __syncthreads();
  const uint32_t cur = sah_levels<LIGHT>(s, b, q, 0u, n, 0u, 0u, 0u, n > SAH_SUBTREE ? SAH_SUBTREE : 0u);
  if (tid == 0u) q.counters[2] = cur;  // the side the subtree workgroups start from
  // leaves fixed at this stage are final; the ranges of the deferred nodes are copied by their own workgroups
  for (uint32_t i = tid; i < n; i += 1024u)
    if (q.item_node[cur][i] == SAH_DONE) b.ids_sorted[i] = q.order[cur][i];
}
// the subtrees below: one workgroup per deferred node, all at once
template <bool LIGHT>
__global__ __launch_bounds__(1024) void k_sah_subtrees(RefitScene s, LbvhBuffers b, SahBuffers q) {
  const uint32_t n_roots = q.counters[1], start = q.counters[2];
  for (uint32_t r = blockIdx.x; r < n_roots; r += gridDim.x) {
    const uint32_t root = q.roots[r], r0 = b.first[root], r1 = b.last[root] + 1u;
    const uint32_t cur = sah_levels<LIGHT>(s, b, q, r0, r1, root, start, 0x40000000u, 0u);
    for (uint32_t i = r0 + threadIdx.x; i < r1; i += 1024u) b.ids_sorted[i] = q.order[cur][i];
    __syncthreads();
  }
}

// ------------------------------------------------------------------ the top of the SAH tree on the whole chip
// k_sah_build runs every level above SAH_SUBTREE-shape nodes in ONE workgroup: sized for 2 * 10^4 instances, not for the 10^5 - 10^6
// triangles of a mesh (hk_rebuild_mesh_tree).  Here a level is five stream-ordered launches over 1024-item chunks, one workgroup per
// chunk - bounds (B), axis (C), buckets (D), split (E), re-order (F) - calling the steps sah_levels calls.  What changes is only how the
// order-free reductions travel:
//   - the segments of the nodes are contiguous, so a chunk whose first and last item share a node belongs to that node alone: its
//     workgroup reduces in LDS (wave_box_accumulate on LDS words) and adds ONE set of atomics per chunk to the node's accumulators -
//     at the top levels that is every chunk, and the hot addresses see a thousand atomics instead of a million;
//   - the stable re-order needs, per item, the count of its bucket in its node BEFORE the chunk.  Only the run at the head of a chunk
//     can have begun earlier, and in each earlier chunk its node is the tail run (first chunk) or the whole chunk: D leaves the six
//     bucket counts of every chunk's head run and tail run in `chunk_counts`, F sums the ones it needs (integers: any order).
// The host launches a FIXED number of levels (it reads nothing back); nodes still unsplit after them go to k_sah_subtrees like the
// small ones, which is correct at any node size.  counters[8 + level] = nodes to split at `level`.
constexpr uint32_t SAH_WIDE_MIN = 32768u;       // shapes from which the top of the tree is built this way
constexpr uint32_t SAH_WIDE_MAX_LEVELS = 48u;   // counters[] holds 64 words
__global__ __launch_bounds__(1024) void k_sahw_setup(LbvhBuffers b, SahBuffers q, uint32_t levels) {
  const uint32_t i = blockIdx.x * 1024u + threadIdx.x;
  if (i < b.n) {
    q.order[0][i] = i;
    q.item_node[0][i] = 0u;
  }
  if (blockIdx.x != 0u) return;
  if (threadIdx.x < 54u) q.acc[threadIdx.x] = sah_acc_init(threadIdx.x);
  if (threadIdx.x < 64u) {
    uint32_t v = 0u;
    if (threadIdx.x == 0u || threadIdx.x == 8u) v = 1u;  // internal nodes allocated; one node to split at level 0
    if (threadIdx.x == 2u) v = levels & 1u;              // the ping-pong side the subtree workgroups start from
    q.counters[threadIdx.x] = v;
  }
  if (threadIdx.x == 0u) {
    b.first[0] = 0u;
    b.last[0] = b.n - 1u;
    b.parent[0] = HK_U32_MAX;
    q.active[0][0] = 0u;
    q.node_level[0] = 0u;
  }
}
// B: bounds of the shapes and of their centres
__global__ __launch_bounds__(1024) void k_sahw_bounds(LbvhBuffers b, SahBuffers q, uint32_t level) {
  __shared__ uint32_t lacc[12];
  const RefitScene none{};
  const uint32_t tid = threadIdx.x, n = b.n, side = level & 1u, c0 = blockIdx.x * 1024u, p = c0 + tid;
  const uint32_t* item_node = q.item_node[side];
  const uint32_t hn = item_node[c0], tn = item_node[min(c0 + 1023u, n - 1u)];
  const bool uniform = hn == tn;
  if (uniform && !sah_splitting(q, hn, level)) return;  // (block-uniform)
  if (tid < 12u) lacc[tid] = sah_acc_init(tid);
  __syncthreads();
  const uint32_t node = p < n ? item_node[p] : SAH_DONE;
  const bool take = sah_splitting(q, node, level);
  sah_item_bounds<false>(none, b, uniform ? lacc : q.acc + (size_t)(take ? node : 0u) * 54u, take, q.order[side], p);
  if (!uniform) return;
  __syncthreads();
  if (tid < 12u) {
    uint32_t* g = q.acc + (size_t)hn * 54u + tid;
    if ((tid % 6u) < 3u) atomicMin(g, lacc[tid]); else atomicMax(g, lacc[tid]);
  }
}
// C: split axis
__global__ __launch_bounds__(256) void k_sahw_axis(SahBuffers q, uint32_t level) {
  const uint32_t n_active = q.counters[8u + level];
  const uint32_t* active = q.active[level & 1u];
  for (uint32_t a = blockIdx.x * 256u + threadIdx.x; a < n_active; a += gridDim.x * 256u) sah_split_axis(q, active[a]);
}
// D: buckets; chunk_counts[12 * chunk ..]: the six bucket counts of the chunk's head run, then of its tail run
__global__ __launch_bounds__(1024) void k_sahw_buckets(LbvhBuffers b, SahBuffers q, uint32_t level, uint32_t* __restrict__ chunk_counts) {
  __shared__ uint32_t lacc[42];  // six bucket boxes, six counts
  __shared__ uint32_t runs[12];
  const RefitScene none{};
  const uint32_t tid = threadIdx.x, n = b.n, side = level & 1u, c0 = blockIdx.x * 1024u, p = c0 + tid;
  const uint32_t* item_node = q.item_node[side];
  const uint32_t hn = item_node[c0], tn = item_node[min(c0 + 1023u, n - 1u)];
  const bool uniform = hn == tn;
  if (uniform && !sah_splitting(q, hn, level)) return;  // (block-uniform; F never reads this chunk's counts)
  if (tid < 42u) lacc[tid] = tid < 36u ? sah_acc_init(tid) : 0u;
  if (tid < 12u) runs[tid] = 0u;
  __syncthreads();
  const uint32_t node = p < n ? item_node[p] : SAH_DONE;
  bool take = sah_splitting(q, node, level);
  float mn[3] = {0, 0, 0}, mx[3] = {0, 0, 0};
  const int bk = sah_item_bucket<false>(none, b, q, node, q.order[side], p, take, mn, mx);
  for (int k6 = 0; k6 < 6; ++k6) {
    const bool mine = take && bk == k6;
    uint32_t* acc = q.acc + (size_t)(mine ? node : 0u) * 54u;
    wave_box_accumulate(uniform ? lacc + 6 * k6 : acc + 12 + 6 * k6, mine, mn, mx, uniform ? lacc + 36 + k6 : acc + 48 + k6);
    if (!uniform) {
      const unsigned long long mh = __ballot(mine && node == hn), mt = __ballot(mine && node == tn);
      if ((tid & 63u) == 0u) {
        if (mh) atomicAdd(&runs[k6], (uint32_t)__popcll(mh));
        if (mt) atomicAdd(&runs[6 + k6], (uint32_t)__popcll(mt));
      }
    }
  }
  __syncthreads();
  if (uniform && tid < 42u) {
    uint32_t* g = q.acc + (size_t)hn * 54u + 12u + tid;
    if (tid >= 36u) atomicAdd(g, lacc[tid]);
    else if ((tid % 6u) < 3u) atomicMin(g, lacc[tid]);
    else atomicMax(g, lacc[tid]);
  }
  if (tid < 12u) chunk_counts[12u * blockIdx.x + tid] = uniform ? lacc[36u + tid % 6u] : runs[tid];
}
// E: the cheapest split, the children (their accumulators start empty: there is no step A here)
__global__ __launch_bounds__(256) void k_sahw_split(LbvhBuffers b, SahBuffers q, uint32_t level, uint32_t defer) {
  const uint32_t n_active = q.counters[8u + level];
  const uint32_t* active = q.active[level & 1u];
  for (uint32_t a = blockIdx.x * 256u + threadIdx.x; a < n_active; a += gridDim.x * 256u) {
    uint32_t child[2];
    sah_split_node(b, q, active[a], level, defer, q.active[(level + 1u) & 1u], &q.counters[9u + level], child);
    for (int side = 0; side < 2; ++side)
      if (child[side] < b.n - 1u)
        for (uint32_t w = 0; w < 54u; ++w) q.acc[(size_t)child[side] * 54u + w] = sah_acc_init(w);
  }
}
// F: stable re-order, bucket by bucket inside every segment
__global__ __launch_bounds__(1024) void k_sahw_reorder(LbvhBuffers b, SahBuffers q, uint32_t level, const uint32_t* __restrict__ chunk_counts) {
  __shared__ uint32_t scan_lds[68];
  __shared__ uint16_t pre[6][1024];
  __shared__ uint32_t carry[6];  // per bucket: items of the head run's node in the chunks before this one
  const uint32_t tid = threadIdx.x, n = b.n, side = level & 1u, c0 = blockIdx.x * 1024u, p = c0 + tid;
  const uint32_t* order = q.order[side];
  const uint32_t* item_node = q.item_node[side];
  uint32_t* order_out = q.order[side ^ 1u];
  uint32_t* item_node_out = q.item_node[side ^ 1u];
  const uint32_t hn = item_node[c0], tn = item_node[min(c0 + 1023u, n - 1u)];
  if (hn == tn && !sah_splitting(q, hn, level)) {  // (block-uniform) nothing of this chunk is split at this level
    if (p < n) {
      order_out[p] = order[p];
      item_node_out[p] = item_node[p];
    }
    return;
  }
  SahItem it;
  const uint32_t h = sah_reorder_scan(q, item_node, c0, n, level, scan_lds, pre, it);
  if (tid < 6u) carry[tid] = 0u;
  __syncthreads();
  if (sah_splitting(q, hn, level) && q.offsets[(size_t)hn * 14u + 13u] != 6u) {  // (block-uniform)
    const uint32_t begin = b.first[hn];
    if (begin < c0 && tid < 1020u) {
      const uint32_t f = begin >> 10, k6 = tid % 6u, g = tid / 6u;  // the node's first chunk: there it is the tail run
      uint32_t sum = g == 0u ? chunk_counts[12u * f + 6u + k6] : 0u;
      for (uint32_t c = f + 1u + g; c < blockIdx.x; c += 170u) sum += chunk_counts[12u * c + k6];  // ... and every chunk between is its alone
      if (sum) atomicAdd(&carry[k6], sum);
    }
  }
  __syncthreads();
  auto carried = [&]() { return h == 0u ? carry[it.bk] : 0u; };  // (only the chunk's head run began earlier)
  sah_reorder_place(b, q, it, p, h, pre, carried, order, order_out, item_node_out);
}
// after the last level: the nodes still unsplit join the deferred ones; leaves fixed so far are final
__global__ __launch_bounds__(256) void k_sahw_finish(LbvhBuffers b, SahBuffers q, uint32_t levels) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x, side = levels & 1u;
  const uint32_t n_left = q.counters[8u + levels];
  for (uint32_t a = i; a < n_left; a += gridDim.x * 256u) q.roots[atomicAdd(&q.counters[1], 1u)] = q.active[side][a];
  if (i < b.n && q.item_node[side][i] == SAH_DONE) b.ids_sorted[i] = q.order[side][i];
}

// ------------------------------------------------------------------ a FOREST of mesh trees in one build (hk_load_scene)
// A scene arrives with thousands of small meshes: one tree build per mesh is six to forty launches each.  Here the triangles of all the
// meshes of a batch form ONE shape array (mesh m owns the positions [tri_begin, tri_begin + n_tris)), and the trees share the arrays of a
// single build: tree nodes are numbered in one space (internal nodes below n - 1, the leaf at position j is n - 1 + j, n = all the
// triangles of the batch), every mesh's root has no parent, and nothing ever crosses a mesh boundary because a node's segment never
// does.  The binned-SAH trees are sah_levels' - the root of mesh m is internal node m; a mesh above SAH_SUBTREE triangles has its top
// levels split by a workgroup of its own (k_forest_tops), then ALL nodes of at most SAH_SUBTREE triangles, whole small meshes among
// them, are built by k_sah_subtrees at once.  The Morton-order trees sort all meshes' codes in one segmented sort.  Boxes bottom-up are
// k_lbvh_boxes; k_forest_emit is k_lbvh_emit with the mesh's own node range as the target and the triangle index local to the mesh.
// The number of launches depends on the mode, not on the number of meshes.
constexpr uint32_t FOREST_UNUSED = 0xFEFEFEFEu;  // parent[] of an internal node id no tree uses: the array is filled with the BYTE 0xFE
// one workgroup per mesh: the triangle boxes, the identity order, the mesh of every position, the root
__global__ __launch_bounds__(256) void k_forest_setup(const ForestMesh* __restrict__ meshes, uint32_t n_meshes, const float4* __restrict__ v0, const float4* __restrict__ v1,
                                                      const float4* __restrict__ v2, float4* __restrict__ tri_lo, float4* __restrict__ tri_hi, uint32_t* __restrict__ item_mesh,
                                                      LbvhBuffers b, SahBuffers q, uint32_t sah) {
  const uint32_t m = blockIdx.x;
  if (m >= n_meshes) return;
  const ForestMesh fm = meshes[m];
  for (uint32_t i = threadIdx.x; i < fm.n_tris; i += 256u) {
    const uint32_t pos = fm.tri_begin + i;
    triangle_box(v0[fm.primitive + i], v1[fm.primitive + i], v2[fm.primitive + i], tri_lo[pos], tri_hi[pos]);
    item_mesh[pos] = m;
    if (sah) {
      q.order[0][pos] = pos;
      q.item_node[0][pos] = fm.n_tris > 1u ? m : SAH_DONE;
    }
    if (fm.n_tris == 1u) {  // a tree of one leaf: nothing to build
      b.ids_sorted[pos] = pos;
      b.leaf_parent[pos] = HK_U32_MAX;
    }
  }
  if (!sah || threadIdx.x != 0u) return;
  if (m == 0u) q.counters[0] = n_meshes;  // internal nodes allocated: the roots (counters[1], [2] were zeroed by the host)
  if (fm.n_tris > 1u) {
    b.first[m] = fm.tri_begin;
    b.last[m] = fm.tri_begin + fm.n_tris - 1u;
    b.parent[m] = HK_U32_MAX;
    if (fm.n_tris <= SAH_SUBTREE) {
      q.node_level[m] = SAH_DONE;
      q.roots[atomicAdd(&q.counters[1], 1u)] = m;
    }
  }
}
// the top levels of every mesh above SAH_SUBTREE triangles, one workgroup each (k_sah_build's part); the range ends on ping-pong side 0,
// where k_sah_subtrees starts from
__global__ __launch_bounds__(1024) void k_forest_tops(const ForestMesh* __restrict__ meshes, const uint32_t* __restrict__ tops, LbvhBuffers b, SahBuffers q) {
  const RefitScene none{};
  const uint32_t m = tops[blockIdx.x];
  const ForestMesh fm = meshes[m];
  const uint32_t r0 = fm.tri_begin, r1 = fm.tri_begin + fm.n_tris;
  const uint32_t cur = sah_levels<false>(none, b, q, r0, r1, m, 0u, 0u, SAH_SUBTREE);
  for (uint32_t i = r0 + threadIdx.x; i < r1; i += 1024u) {
    const uint32_t node = q.item_node[cur][i], shape = q.order[cur][i];
    if (cur != 0u) {
      q.item_node[0][i] = node;
      q.order[0][i] = shape;
    }
    if (node == SAH_DONE) b.ids_sorted[i] = shape;  // leaves fixed at this stage are final
  }
}
// Morton-order trees: the centre bounds of every mesh (one workgroup each), the codes inside them, Karras' hierarchy per segment
__global__ __launch_bounds__(256) void k_forest_lbvh_bounds(const ForestMesh* __restrict__ meshes, LbvhBuffers b, float* __restrict__ mesh_bounds) {
  const RefitScene none{};
  const ForestMesh fm = meshes[blockIdx.x];
  float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (uint32_t i = threadIdx.x; i < fm.n_tris; i += 256u) {
    f3 lo, hi;
    lbvh_shape_box<false>(none, b, fm.tri_begin + i, lo, hi);
    centre_bounds_add(lo, hi, mn, mx);
  }
  block_centre_bounds<4>(mn, mx, mesh_bounds + 6u * blockIdx.x);
}
__global__ __launch_bounds__(256) void k_forest_lbvh_codes(const uint32_t* __restrict__ item_mesh, const float* __restrict__ mesh_bounds, LbvhBuffers b) {
  const RefitScene none{};
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= b.n) return;
  f3 lo, hi;
  lbvh_shape_box<false>(none, b, i, lo, hi);
  b.codes[i] = morton_code(lo, hi, mesh_bounds + 6u * item_mesh[i]);
  b.ids[i] = i;
}
// one thread per position: internal node i of the position's mesh, inside the mesh's segment
__global__ __launch_bounds__(256) void k_forest_lbvh_hierarchy(const ForestMesh* __restrict__ meshes, const uint32_t* __restrict__ item_mesh, LbvhBuffers b) {
  const uint32_t g = blockIdx.x * 256u + threadIdx.x;
  if (g >= b.n) return;
  const ForestMesh fm = meshes[item_mesh[g]];
  const int n = (int)fm.n_tris, i = (int)(g - fm.tri_begin);
  if (i >= n - 1) return;
  karras_node(b, fm.tri_begin, n, i);
}
// one thread per tree node and ordering (emit_tree_node), into the node range of the node's mesh, with links and triangle indices local
// to the mesh.  parent[] was filled with FOREST_UNUSED before the build
__global__ __launch_bounds__(256) void k_forest_emit(const ForestMesh* __restrict__ meshes, const uint32_t* __restrict__ item_mesh, LbvhBuffers b, float4* nodes,
                                                     size_t ord_stride /* float4 between orderings */, uint32_t orderings) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x, n = b.n, total = 2u * n - 1u;
  if (t >= total * orderings) return;
  const uint32_t o = t / total, v = t - o * total;
  const bool leaf = v >= n - 1u;
  const uint32_t p = leaf ? b.leaf_parent[v - (n - 1u)] : b.parent[v];
  if (!leaf && (p == FOREST_UNUSED || p == HK_U32_MAX)) return;  // no such node; a root has no navigator
  const ForestMesh fm = meshes[item_mesh[leaf ? v - (n - 1u) : b.first[v]]];
  float4* nlo = nodes + (size_t)o * ord_stride + 2u * (size_t)fm.node_offset;
  const uint32_t shape = leaf ? b.ids_sorted[v - (n - 1u)] - fm.tri_begin : 0u;
  emit_tree_node<true>(b, v, p, o, shape, fm.n_tris, nlo, nlo + 1, 2u);
}

}  // namespace hkd

namespace hk {
using namespace hkd;

// the refit of a mesh tree is the last two steps of a tree build over its fixed topology: boxes bottom-up (k_lbvh_boxes: leaf boxes =
// the triangle boxes, every internal node by the second child to arrive, child order per ordering by the rule of hk_bvh_rethread with
// ordering 0 kept as it is), then every node written at its place in every ordering (k_lbvh_emit)
void launch_mesh_tree_refit(hipStream_t st, const MeshTree& t, float4* lo, size_t ord_stride, uint32_t orderings) {
  const LbvhBuffers b = mesh_refit_buffers(t);
  if (t.n > 1u) (void)hipMemsetAsync(t.arrived, 0, (size_t)(t.n - 1u) * 4, st);
  const RefitScene none{};
  hipLaunchKernelGGL((k_lbvh_boxes<false>), dim3((t.n + 255u) / 256u), dim3(256), 0, st, none, b);
  const uint32_t threads = (2u * t.n - 1u) * orderings;
  hipLaunchKernelGGL(k_lbvh_emit, dim3((threads + 255u) / 256u), dim3(256), 0, st, b, lo, lo + 1, 2u, ord_stride, orderings);
}
// ... of every item of a batch, in two launches
void launch_deform_tree_refit(hipStream_t st, const DeformItem* items, const SegmentBlock* triangle_blocks, uint32_t n_triangle_blocks, const SegmentBlock* node_blocks,
                              uint32_t n_node_blocks, size_t ord_stride, uint32_t orderings) {
  if (!n_triangle_blocks || !n_node_blocks) return;
  hipLaunchKernelGGL(k_deform_boxes, dim3(n_triangle_blocks), dim3(256), 0, st, items, triangle_blocks);
  hipLaunchKernelGGL(k_deform_emit, dim3(n_node_blocks), dim3(256), 0, st, items, node_blocks, ord_stride, orderings);
}

// ---- the scratch of a build: ONE description of its layout.  Sizing carves from a null base and returns the end; the builds carve
// the real allocation with the same function, so the two cannot disagree.
static size_t radix_sort_temp(uint32_t n) {
  size_t temp = 0;
  (void)rocprim::radix_sort_pairs(nullptr, temp, (const uint32_t*)nullptr, (uint32_t*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr, (size_t)n, 0, 30);
  return (temp + 255) & ~(size_t)255;
}
static size_t forest_sort_temp(uint32_t n_tris, uint32_t n_meshes) {
  size_t temp = 0;
  (void)rocprim::segmented_radix_sort_pairs(nullptr, temp, (const uint32_t*)nullptr, (uint32_t*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr, n_tris, n_meshes,
                                            (const uint32_t*)nullptr, (const uint32_t*)nullptr, 0, 30);
  return (temp + 255) & ~(size_t)255;
}
struct TreeScratch {
  LbvhBuffers b;   // (n, the shapes and keep_order0 are the build's to fill in)
  SahBuffers q;    // the binned-SAH build's arrays
  void* sort_temp;         // the Morton-order build's
  uint32_t* chunk_counts;  // the multi-workgroup SAH top's: 12 words per 1024-item chunk
  // a forest build's extras
  float4 *tri_lo, *tri_hi;
  uint32_t* item_mesh;
  ForestMesh* meshes;
  uint32_t *tops, *seg_begin, *seg_end;
  float* mesh_bounds;
};
constexpr int TREE_MODE_EITHER = 2;  // a single tree's scratch serves both modes: callers size it once, before they know the mode
// Carves the scratch of a build over n shapes out of `base` (nullptr: sizes only) and returns its end offset.  mode 0: the Morton-order
// build (with `sort_temp` bytes for the sort), 1: the binned-SAH build, TREE_MODE_EITHER: both.  `forest`: a forest of n_meshes meshes,
// with its triangle boxes, item_mesh and per-mesh arrays.  Array lengths are rounded up to 64 entries: every array starts on
// a 256-byte boundary.
static size_t carve_tree_scratch(TreeScratch& t, void* base, uint32_t n, int mode, size_t sort_temp, bool forest, uint32_t n_meshes) {
  const size_t nn = ((size_t)n + 63) & ~(size_t)63, mm = ((size_t)n_meshes + 63) & ~(size_t)63;
  size_t at = 0;
  auto take = [&](size_t bytes) { void* p = base ? (uint8_t*)base + at : nullptr; at += bytes; return p; };
  auto u32 = [&](size_t count) { return (uint32_t*)take(count * 4); };
  t = TreeScratch{};
  LbvhBuffers& b = t.b;
  b.bounds = (float*)take(256);
  if (mode != 1) t.sort_temp = take(sort_temp);
  b.codes = u32(nn); b.codes_sorted = u32(nn); b.ids = u32(nn); b.ids_sorted = u32(nn);
  b.parent = u32(nn); b.left = u32(nn); b.right = u32(nn); b.first = u32(nn); b.last = u32(nn); b.leaf_parent = u32(nn); b.arrived = u32(nn);
  b.swap = (uint8_t*)u32(nn);  // (one byte per node, padded)
  b.node_lo = (float4*)take(2 * nn * 16);  // 2n - 1 tree nodes
  b.node_hi = (float4*)take(2 * nn * 16);
  if (forest) {
    t.tri_lo = (float4*)take(nn * 16); t.tri_hi = (float4*)take(nn * 16);
    t.item_mesh = u32(nn);
    t.meshes = (ForestMesh*)take(mm * sizeof(ForestMesh));
    t.tops = u32(mm); t.seg_begin = u32(mm); t.seg_end = u32(mm);
    t.mesh_bounds = (float*)u32(6 * mm);
  }
  if (mode != 0) {
    SahBuffers& q = t.q;
    q.order[0] = b.codes; q.order[1] = b.codes_sorted;  // (the Morton arrays are free in this mode)
    q.item_node[0] = b.ids; q.item_node[1] = u32(nn);
    q.item_bucket = (uint8_t*)u32(nn);                  // (one byte per item, padded)
    q.active[0] = u32(nn); q.active[1] = u32(nn);
    q.acc = u32(nn * 54); q.split = (float*)u32(nn * 4); q.offsets = u32(nn * 14);
    q.node_level = u32(nn); q.roots = u32(nn);
    q.counters = (uint32_t*)b.bounds;                   // (256 B, unused by this mode)
  }
  if (!forest) t.chunk_counts = u32((nn / 1024 + 1) * 12);  // (a forest never takes the multi-workgroup top)
  return at;
}

size_t lbvh_scratch_bytes(uint32_t n) {
  TreeScratch t;
  return carve_tree_scratch(t, nullptr, n, TREE_MODE_EITHER, radix_sort_temp(n), false, 0u);
}
int launch_tree_build(hipStream_t st, const TreeBuild& d) {
  const uint32_t n = d.n;
  if (n == 0) return 0;
  const bool light = d.box_lo == nullptr;
  if ((d.keep && !d.mesh_tree) || (light && !d.scene) || (!light && !d.box_hi)) return 1;  // (only a mesh tree has a topology to keep; the emitters are the scene's)
  const RefitScene none{};
  const RefitScene& s = d.scene ? *d.scene : none;
  uint32_t launched = 2u;  // boxes, emit
  const size_t temp = radix_sort_temp(n);
  TreeScratch t;
  (void)carve_tree_scratch(t, d.scratch, n, TREE_MODE_EITHER, temp, false, 0u);
  const size_t nn = ((size_t)n + 63) & ~(size_t)63;
  LbvhBuffers& b = t.b;
  const SahBuffers& q = t.q;
  b.n = n;
  b.box_lo = d.box_lo; b.box_hi = d.box_hi;
  b.keep_order0 = (d.mode == 1 || d.mesh_tree) ? 1u : 0u;  // (a mesh tree's ordering 0 is what its refit keeps: left before right)
  (void)hipMemsetAsync(b.arrived, 0, nn * 4, st);
  (void)hipMemsetAsync(b.swap, 0, nn * 4, st);
  const dim3 per_shape((n + 255u) / 256u);
  if (d.mode == 1) {
    const dim3 subtrees((unsigned)std::min<size_t>(std::max<size_t>(n / 2, 1), 4096));
    launched += n > SAH_SUBTREE ? 2u : 1u;
    if (d.mesh_tree && n >= SAH_WIDE_MIN && !d.one_workgroup_top) {  // (mesh trees only: the instance tree and the light tree keep the one-workgroup top at any size)
      // the levels a balanced tree needs down to SAH_SUBTREE shapes per node, and six more for the lopsided splits of a real one
      uint32_t levels = 6u;
      while (((size_t)SAH_SUBTREE << (levels - 6u)) < n) ++levels;
      levels = std::min(levels, SAH_WIDE_MAX_LEVELS);
      const dim3 chunks((n + 1023u) / 1024u);
      launched += 1u + 5u * levels;
      hipLaunchKernelGGL(k_sahw_setup, chunks, dim3(1024), 0, st, b, q, levels);
      for (uint32_t level = 0; level < levels; ++level) {
        const dim3 per_node((unsigned)std::min<size_t>(((size_t)1 << std::min(level, 20u)) / 256 + 1, 256));  // (at most 2^level nodes)
        hipLaunchKernelGGL(k_sahw_bounds, chunks, dim3(1024), 0, st, b, q, level);
        hipLaunchKernelGGL(k_sahw_axis, per_node, dim3(256), 0, st, q, level);
        hipLaunchKernelGGL(k_sahw_buckets, chunks, dim3(1024), 0, st, b, q, level, t.chunk_counts);
        hipLaunchKernelGGL(k_sahw_split, per_node, dim3(256), 0, st, b, q, level, SAH_SUBTREE);
        hipLaunchKernelGGL(k_sahw_reorder, chunks, dim3(1024), 0, st, b, q, level, (const uint32_t*)t.chunk_counts);
      }
      hipLaunchKernelGGL(k_sahw_finish, per_shape, dim3(256), 0, st, b, q, levels);
      hipLaunchKernelGGL((k_sah_subtrees<false>), subtrees, dim3(1024), 0, st, s, b, q);
    } else {
      hipLaunchKernelGGL(light ? k_sah_build<true> : k_sah_build<false>, dim3(1), dim3(1024), 0, st, s, b, q);
      if (n > SAH_SUBTREE) hipLaunchKernelGGL(light ? k_sah_subtrees<true> : k_sah_subtrees<false>, subtrees, dim3(1024), 0, st, s, b, q);
    }
  } else {
    hipLaunchKernelGGL(light ? k_lbvh_bounds<true> : k_lbvh_bounds<false>, dim3(1), dim3(1024), 0, st, s, b);
    hipLaunchKernelGGL(light ? k_lbvh_codes<true> : k_lbvh_codes<false>, per_shape, dim3(256), 0, st, s, b);
    size_t sort_bytes = temp;
    if (rocprim::radix_sort_pairs(t.sort_temp, sort_bytes, (const uint32_t*)b.codes, b.codes_sorted, (const uint32_t*)b.ids, b.ids_sorted, (size_t)n, 0, 30, st) != hipSuccess) return 1;
    if (n > 1) hipLaunchKernelGGL(k_lbvh_hierarchy, dim3((n + 254u) / 256u), dim3(256), 0, st, b);
    launched += 4u;  // (the sort counted as one)
  }
  if (d.launches) *d.launches += launched;
  hipLaunchKernelGGL(light ? k_lbvh_boxes<true> : k_lbvh_boxes<false>, per_shape, dim3(256), 0, st, s, b);
  const uint32_t threads = (2u * n - 1u) * d.orderings;
  hipLaunchKernelGGL(k_lbvh_emit, dim3((threads + 255u) / 256u), dim3(256), 0, st, b, d.lo, d.hi, d.stride, d.ord_stride ? d.ord_stride : (size_t)(3u * n - 2u) * d.stride,
                     d.orderings);
  if (d.keep) {  // the topology a later refit of this tree climbs (launch_mesh_tree_refit)
    const MeshTree* keep = d.keep;
    const size_t ni = (size_t)(n - 1u) * 4;
    const std::pair<uint32_t*, const uint32_t*> planes[5] = {{keep->parent, b.parent}, {keep->left, b.left}, {keep->right, b.right}, {keep->first, b.first}, {keep->last, b.last}};
    for (const auto& pl : planes)
      if (ni) (void)hipMemcpyAsync(pl.first, pl.second, ni, hipMemcpyDeviceToDevice, st);
    if (ni) (void)hipMemcpyAsync(keep->leaf_parent, b.leaf_parent, (size_t)n * 4, hipMemcpyDeviceToDevice, st);
    (void)hipMemcpyAsync(keep->leaf_shape, b.ids_sorted, (size_t)n * 4, hipMemcpyDeviceToDevice, st);
  }
  return hipGetLastError() == hipSuccess ? 0 : 1;
}

// ---- a forest of mesh trees (hk_load_scene): scratch of one batch, and the build of every mesh of the batch into its own node range
static_assert(HK_FOREST_MESH_MAX_TRIANGLES + 1u == SAH_WIDE_MIN, "the forest takes every mesh below the multi-workgroup build");
size_t forest_scratch_bytes(uint32_t n_tris, uint32_t n_meshes, int mode) {
  TreeScratch t;
  return carve_tree_scratch(t, nullptr, n_tris, mode, mode == 1 ? 0 : forest_sort_temp(n_tris, n_meshes), true, n_meshes);
}
int launch_forest_build(hipStream_t st, int mode, const ForestMesh* meshes, uint32_t n_meshes, uint32_t n_tris, const float4* v0, const float4* v1, const float4* v2, void* scratch,
                        float4* nodes, uint32_t orderings, size_t ord_stride, uint32_t* launches) {
  if (n_meshes == 0 || n_tris == 0) return 0;
  const uint32_t n = n_tris;
  const size_t nn = ((size_t)n + 63) & ~(size_t)63;
  size_t temp = mode == 1 ? 0 : forest_sort_temp(n, n_meshes);
  TreeScratch t;
  (void)carve_tree_scratch(t, scratch, n, mode, temp, true, n_meshes);
  LbvhBuffers& b = t.b;
  const SahBuffers& q = t.q;
  b.n = n;
  b.box_lo = t.tri_lo; b.box_hi = t.tri_hi;
  b.keep_order0 = 1u;  // (a mesh tree's ordering 0 is what its refit keeps: left before right)
  // (pageable sources: the copies have left the host buffers when the calls return)
  if (hipMemcpyAsync(t.meshes, meshes, (size_t)n_meshes * sizeof(ForestMesh), hipMemcpyHostToDevice, st) != hipSuccess) return 1;
  (void)hipMemsetAsync(b.arrived, 0, nn * 4, st);
  (void)hipMemsetAsync(b.swap, 0, nn * 4, st);
  (void)hipMemsetAsync(b.parent, (int)(FOREST_UNUSED & 0xFFu), nn * 4, st);
  (void)hipMemsetAsync(b.leaf_parent, 0xFF, nn * 4, st);
  (void)hipMemsetAsync(b.bounds, 0, 256, st);        // (the SAH build's counters)
  const RefitScene none{};
  const dim3 per_shape((n + 255u) / 256u);
  const ForestMesh* d_meshes = t.meshes;
  const uint32_t* item_mesh = t.item_mesh;
  uint32_t launched = 0u;
  if (mode == 1) {
    std::vector<uint32_t> tops;
    for (uint32_t m = 0; m < n_meshes; ++m)
      if (meshes[m].n_tris > SAH_SUBTREE) tops.push_back(m);
    if (!tops.empty() && hipMemcpyAsync(t.tops, tops.data(), tops.size() * 4, hipMemcpyHostToDevice, st) != hipSuccess) return 1;
    hipLaunchKernelGGL(k_forest_setup, dim3(n_meshes), dim3(256), 0, st, d_meshes, n_meshes, v0, v1, v2, t.tri_lo, t.tri_hi, t.item_mesh, b, q, 1u);
    if (!tops.empty()) hipLaunchKernelGGL(k_forest_tops, dim3((unsigned)tops.size()), dim3(1024), 0, st, d_meshes, (const uint32_t*)t.tops, b, q);
    hipLaunchKernelGGL((k_sah_subtrees<false>), dim3((unsigned)std::min<size_t>(std::max<size_t>(n / 2, 1), 4096)), dim3(1024), 0, st, none, b, q);
    launched += tops.empty() ? 2u : 3u;
  } else {
    std::vector<uint32_t> seg(2 * (size_t)n_meshes);
    for (uint32_t m = 0; m < n_meshes; ++m) {
      seg[m] = meshes[m].tri_begin;
      seg[n_meshes + m] = meshes[m].tri_begin + meshes[m].n_tris;
    }
    if (hipMemcpyAsync(t.seg_begin, seg.data(), (size_t)n_meshes * 4, hipMemcpyHostToDevice, st) != hipSuccess) return 1;
    if (hipMemcpyAsync(t.seg_end, seg.data() + n_meshes, (size_t)n_meshes * 4, hipMemcpyHostToDevice, st) != hipSuccess) return 1;
    hipLaunchKernelGGL(k_forest_setup, dim3(n_meshes), dim3(256), 0, st, d_meshes, n_meshes, v0, v1, v2, t.tri_lo, t.tri_hi, t.item_mesh, b, q, 0u);
    hipLaunchKernelGGL(k_forest_lbvh_bounds, dim3(n_meshes), dim3(256), 0, st, d_meshes, b, t.mesh_bounds);
    hipLaunchKernelGGL(k_forest_lbvh_codes, per_shape, dim3(256), 0, st, item_mesh, (const float*)t.mesh_bounds, b);
    if (rocprim::segmented_radix_sort_pairs(t.sort_temp, temp, (const uint32_t*)b.codes, b.codes_sorted, (const uint32_t*)b.ids, b.ids_sorted, n, n_meshes,
                                            (const uint32_t*)t.seg_begin, (const uint32_t*)t.seg_end, 0, 30, st) != hipSuccess)
      return 1;
    hipLaunchKernelGGL(k_forest_lbvh_hierarchy, per_shape, dim3(256), 0, st, d_meshes, item_mesh, b);
    launched += 5u;  // (the sort counted as one)
  }
  hipLaunchKernelGGL((k_lbvh_boxes<false>), per_shape, dim3(256), 0, st, none, b);
  const uint32_t threads = (2u * n - 1u) * orderings;
  hipLaunchKernelGGL(k_forest_emit, dim3((threads + 255u) / 256u), dim3(256), 0, st, d_meshes, item_mesh, b, nodes, ord_stride, orderings);
  launched += 2u;
  if (launches) *launches += launched;
  return hipGetLastError() == hipSuccess ? 0 : 1;
}

}  // namespace hk
