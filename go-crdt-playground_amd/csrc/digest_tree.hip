// The digest tree: a hash tree of fan-out 16 over a per-document digest array,
// and the two device calls of a level-by-level descent (crdt_digest_tree_async,
// crdt_digest_tree_children_async, crdt_digest_tree_diff_async;
// include/crdtgpu.h, "digest trees").  The terms are digest_hash.hpp's.
//
// Build.  One lane per child, one 16-lane row of a wavefront per node: a lane
// reads both words of its child with one 16 B load (a wavefront reads 1 KB
// contiguous and owns four nodes), salts them with its slot, the row sums each
// word with four xor steps that never leave the row, and lane 0 of the row
// stores the node with one 16 B store.  A lane past the level contributes zero,
// so the partial last node needs no other path.  Sums of integers commute: the
// words are bit for bit crdt_digest_tree_host's.  Launches:
//
//   tree_level_kernel   one level, one thread per child slot of its nodes.
//   tree_top_kernel     one workgroup: every level from the first whose children
//       number kTreeTopChildren or fewer up to the root, one after the other with
//       a barrier between (the nodes a level wrote are the next one's children).
//       `fuse == 0` (crdt_ctx_set_option "digest_tree_fuse") launches
//       tree_level_kernel for those levels too: the A/B of DESIGN.md §5.
//
// No incremental update: the tree is rebuilt whole from the digest array, which
// crdt_awset_digest_idx_async keeps current (17 MB of streaming reads at 2^20
// documents; re-deriving the ancestors of a worklist touches nearly every
// level-1 node from about 5 % random documents on).
//
// Children.  tree_children_kernel: a gather, one lane per (listed parent, slot),
// 16 B load and store; a slot past the level, and every slot of a parent that is
// no node (kErrIndex), is written as zeros.
//
// Diff.  The listed parents are cut into chunks of kTreeChunk; three launches,
// ordered by their kernel boundaries alone, as scatter.hip's scan:
//
//   tree_diff_count_kernel     workgroup c: one row per listed parent, a ballot
//       per wavefront of the listed children; parts[c] = children listed,
//       parts[n_parts + c] / parts[2 n_parts + c] = children with e / with s.
//       Reports every error of the call.
//   tree_diff_partials_kernel  one workgroup: parts[c] becomes its exclusive
//       prefix; *n_out and the summary.
//   tree_diff_emit_kernel      workgroup c computes the same flags again
//       (tree_diff_flag, shared with the count) and writes the listed children at
//       parts[c] + their rank in the chunk, in (parent, slot) order: ascending
//       when the parents are.  No atomic decides a position.
#include "crdt_device.hpp"
#include "digest_hash.hpp"
#include "merge_block.hpp"

namespace crdt {

constexpr int kTreeNT = 256;
constexpr uint32_t kTreeTopNT = 1024;
constexpr uint32_t kTreeTopChildren = 4096;  // levels of this many children or fewer: tree_top_kernel
constexpr uint32_t kTreeRows = kTreeNT / kDigTreeFanout;  // 16 listed parents per workgroup step
constexpr int kTreeSteps = 4;
constexpr uint32_t kTreeChunk = kTreeRows * kTreeSteps;  // 64 listed parents per scan chunk
constexpr int kTreePartNT = 1024;

typedef unsigned long long ull;

__device__ __forceinline__ uint64_t tree_row_sum(uint64_t w) {
#pragma unroll
    for (int o = (int)kDigTreeFanout / 2; o > 0; o >>= 1) w += (uint64_t)__shfl_xor((ull)w, o);
    return w;
}

__device__ __forceinline__ void tree_load(const uint64_t* a, uint64_t i, uint32_t vec, uint64_t& w0, uint64_t& w1) {
    if (vec) {
        const ulonglong2 x = *reinterpret_cast<const ulonglong2*>(a + 2 * i);
        w0 = x.x;
        w1 = x.y;
    } else {
        w0 = a[2 * i];
        w1 = a[2 * i + 1];
    }
}

__device__ __forceinline__ void tree_store(uint64_t* a, uint64_t i, uint32_t vec, uint64_t w0, uint64_t w1) {
    if (vec) {
        *reinterpret_cast<ulonglong2*>(a + 2 * i) = make_ulonglong2(w0, w1);
    } else {
        a[2 * i] = w0;
        a[2 * i + 1] = w1;
    }
}

// Child slot i of the level (i may lie past it: then only the row sums are
// joined).  Every lane of a wavefront calls this together.
__device__ __forceinline__ void tree_node_step(const uint64_t* child, uint32_t n_child, uint64_t* node, uint64_t i,
                                               uint32_t vec_in, uint32_t vec_out) {
    const uint32_t c = (uint32_t)(i & (kDigTreeFanout - 1));
    uint64_t t0 = 0, t1 = 0;
    if (i < n_child) {
        uint64_t w0, w1;
        tree_load(child, i, vec_in, w0, w1);
        t0 = dig_tree_term(w0, c);
        t1 = dig_tree_term(w1, c);
    }
    t0 = tree_row_sum(t0);
    t1 = tree_row_sum(t1);
    if (c == 0 && i < n_child) {  // (the node exists iff its first child does)
        const uint64_t left = (uint64_t)n_child - i;
        const uint32_t cnt = left < kDigTreeFanout ? (uint32_t)left : kDigTreeFanout;
        tree_store(node, i / kDigTreeFanout, vec_out, dig_tree_node(t0, cnt), dig_tree_node(t1, cnt));
    }
}

__global__ __launch_bounds__(kTreeNT) void tree_level_kernel(const uint64_t* child, uint32_t n_child, uint64_t* node,
                                                             uint32_t vec_in, uint32_t vec_out) {
    tree_node_step(child, n_child, node, (uint64_t)blockIdx.x * kTreeNT + threadIdx.x, vec_in, vec_out);
}

struct TreeTopArgs {
    const uint64_t* child;  // the first level's children
    uint64_t* node[kDigTreeMaxLevels];
    uint32_t n_child[kDigTreeMaxLevels];
    uint32_t n_levels;
    uint32_t vec_in, vec_out;  // vec_in: of `child`; the later levels read what vec_out wrote
};

__global__ __launch_bounds__(kTreeTopNT) void tree_top_kernel(TreeTopArgs a) {
    const uint64_t* child = a.child;
    uint32_t vec_in = a.vec_in;
    for (uint32_t l = 0; l < a.n_levels; ++l) {
        const uint32_t n = a.n_child[l];  // (<= kTreeTopChildren)
        const uint32_t slots = (n + kDigTreeFanout - 1) / kDigTreeFanout * kDigTreeFanout;
        for (uint32_t base = 0; base < slots; base += kTreeTopNT)  // (uniform: whole wavefronts step together)
            tree_node_step(child, n, a.node[l], (uint64_t)base + threadIdx.x, vec_in, a.vec_out);
        __threadfence_block();
        __syncthreads();
        child = a.node[l];
        vec_in = a.vec_out;
    }
}

static bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// n_docs == 0: nothing is launched.
hipError_t launch_digest_tree(const uint64_t* digest, uint32_t n_docs, uint64_t* tree, bool fuse, hipStream_t stream) {
    if (n_docs == 0) return hipSuccess;
    uint32_t nodes[9], off[9];
    const int L = dig_tree_layout(n_docs, nodes, off);
    // (every level starts an even number of words into the tree: one alignment for all)
    const uint32_t vec_tree = aligned(tree, 16);
    const uint64_t* child = digest;
    uint32_t vec_in = aligned(digest, 16);
    int l = 1;
    for (; l <= L && !(fuse && nodes[l - 1] <= kTreeTopChildren); ++l) {
        uint64_t* node = tree + 2 * (size_t)off[l];
        const uint32_t grid = (uint32_t)(((uint64_t)nodes[l] * kDigTreeFanout + kTreeNT - 1) / kTreeNT);
        hipLaunchKernelGGL(tree_level_kernel, dim3(grid), dim3(kTreeNT), 0, stream, child, nodes[l - 1], node, vec_in,
                           vec_tree);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        child = node;
        vec_in = vec_tree;
    }
    if (l > L) return hipSuccess;
    TreeTopArgs a{};
    a.child = child;
    a.vec_in = vec_in;
    a.vec_out = vec_tree;
    for (; l <= L; ++l) {
        a.node[a.n_levels] = tree + 2 * (size_t)off[l];
        a.n_child[a.n_levels] = nodes[l - 1];
        ++a.n_levels;
    }
    hipLaunchKernelGGL(tree_top_kernel, dim3(1), dim3(kTreeTopNT), 0, stream, a);
    return hipGetLastError();
}

// ---- the descent -------------------------------------------------------------

struct TreeList {
    const uint64_t* level;  // the children: [2 * n_level]
    uint32_t n_level;
    const uint32_t* parents;    // NULL: the identity
    const uint32_t* n_parents;  // NULL: n_max
    uint32_t n_max;
    uint32_t vec_level;
};

// Parents listed, clamped to n_max.
__device__ __forceinline__ uint32_t tree_list_n(const TreeList& a, uint32_t& err) {
    uint32_t n = a.n_parents ? *a.n_parents : a.n_max;
    if (n > a.n_max) {
        err |= kErrCapacity;
        n = a.n_max;
    }
    return n;
}

// Listed parent j < the list's length: its node index, false when it is no node.
__device__ __forceinline__ bool tree_list_parent(const TreeList& a, uint32_t j, uint32_t& p, uint32_t& err) {
    p = a.parents ? a.parents[j] : j;
    if ((uint64_t)p * kDigTreeFanout >= a.n_level) {  // p >= ceil(n_level / 16)
        err |= kErrIndex;
        return false;
    }
    return true;
}

__global__ __launch_bounds__(kTreeNT) void tree_children_kernel(TreeList a, uint64_t* out, uint32_t vec_out,
                                                                uint32_t* status) {
    uint32_t err = 0;
    const uint32_t n_list = tree_list_n(a, err);
    const uint64_t i = (uint64_t)blockIdx.x * kTreeNT + threadIdx.x;  // slot 16 j + c of out
    const uint32_t j = (uint32_t)(i / kDigTreeFanout), c = (uint32_t)(i & (kDigTreeFanout - 1));
    if (j < n_list) {
        uint32_t p;
        uint64_t w0 = 0, w1 = 0;
        if (tree_list_parent(a, j, p, err)) {
            const uint64_t child = (uint64_t)p * kDigTreeFanout + c;
            if (child < a.n_level) tree_load(a.level, child, a.vec_level, w0, w1);
        }
        tree_store(out, i, vec_out, w0, w1);
    }
    flag_error(status, err);
}

// n_max == 0: nothing is launched.
hipError_t launch_digest_tree_children(const uint64_t* level, uint32_t n_level, const uint32_t* parents,
                                       const uint32_t* n_parents, uint32_t n_max, uint64_t* out, uint32_t* status,
                                       hipStream_t stream) {
    if (n_max == 0) return hipSuccess;
    const TreeList a{level, n_level, parents, n_parents, n_max, aligned(level, 16)};
    const uint32_t grid = (uint32_t)(((uint64_t)n_max * kDigTreeFanout + kTreeNT - 1) / kTreeNT);
    hipLaunchKernelGGL(tree_children_kernel, dim3(grid), dim3(kTreeNT), 0, stream, a, out, (uint32_t)aligned(out, 16),
                       status);
    return hipGetLastError();
}

struct TreeDiffArgs {
    TreeList mine;
    const uint64_t* theirs;  // [2 * 16 * listed parents], as tree_children_kernel packs them
    uint32_t vec_theirs;
    uint32_t leaf, mask;
    uint32_t* idx_out;
    uint8_t* flags_out;  // NULL: not written
    uint32_t* n_out;
    uint32_t out_max;
    uint32_t* summary;  // NULL: not written
};

// Slot c of listed parent j (j may lie past the list of n_list parents): the
// child's index and its flag, 0 when it is equal, past the level or no child at
// all.  e / s: word 0 / word 1 differs.  The count and the emit pass both call
// this and nothing else.
__device__ __forceinline__ uint32_t tree_diff_flag(const TreeDiffArgs& a, uint32_t n_list, uint32_t j, uint32_t c,
                                                   uint32_t& child, bool& e, bool& s, uint32_t& err) {
    e = s = false;
    child = 0;
    if (j >= n_list) return 0;
    uint32_t p;
    if (!tree_list_parent(a.mine, j, p, err)) return 0;
    // strictly ascending: each listed parent against the one before it
    if (a.mine.parents && j > 0 && a.mine.parents[j - 1] >= p) err |= kErrIndex;
    const uint64_t ch = (uint64_t)p * kDigTreeFanout + c;
    if (ch >= a.mine.n_level) return 0;
    child = (uint32_t)ch;
    uint64_t m0, m1, t0, t1;
    tree_load(a.mine.level, ch, a.mine.vec_level, m0, m1);
    tree_load(a.theirs, (uint64_t)j * kDigTreeFanout + c, a.vec_theirs, t0, t1);
    e = m0 != t0;
    s = m1 != t1;
    if (a.leaf) return e ? CRDT_DIG_ELEMENTS : (s ? CRDT_DIG_STATE : 0u);
    return (e ? 1u : 0u) | (s ? 2u : 0u);
}

__global__ __launch_bounds__(kTreeNT) void tree_diff_count_kernel(TreeDiffArgs a, uint32_t* parts, uint32_t n_parts,
                                                                  uint32_t* status) {
    __shared__ uint32_t s_cnt[3][kTreeNT / 64];
    const uint32_t t = threadIdx.x, w = t >> 6;
    uint32_t err = 0;
    const uint32_t n_list = tree_list_n(a.mine, err);
    uint32_t listed = 0, n_e = 0, n_s = 0;  // (the same in every lane of a wavefront)
#pragma unroll
    for (int k = 0; k < kTreeSteps; ++k) {
        const uint32_t j = blockIdx.x * kTreeChunk + (uint32_t)k * kTreeRows + t / kDigTreeFanout;
        uint32_t child;
        bool e, s;
        const uint32_t f = tree_diff_flag(a, n_list, j, t & (kDigTreeFanout - 1), child, e, s, err);
        listed += popc(ballot((f & a.mask) != 0u));
        n_e += popc(ballot(e));
        n_s += popc(ballot(a.leaf ? (s && !e) : s));
    }
    if ((t & 63u) == 0) {
        s_cnt[0][w] = listed;
        s_cnt[1][w] = n_e;
        s_cnt[2][w] = n_s;
    }
    __syncthreads();
    if (t < 3) {
        uint32_t sum = 0;
#pragma unroll
        for (int x = 0; x < kTreeNT / 64; ++x) sum += s_cnt[t][x];
        parts[(size_t)t * n_parts + blockIdx.x] = sum;
    }
    flag_error(status, err);
}

// One workgroup: parts[0 .. n_parts) -> exclusive prefixes; the totals of all
// three rows into *n_out and the summary.  n_parts == 0: zeros.  The sums are
// u32, as *n_out is: a level has n_level < 2^32 children and a strictly
// ascending list names each at most once, so they cannot wrap.  A list that is
// not ascending may name children again; it is reported (kErrIndex) and its
// counts mean nothing then, while every write stays below out_max.
__global__ __launch_bounds__(kTreePartNT) void tree_diff_partials_kernel(uint32_t* parts, uint32_t n_parts,
                                                                         TreeDiffArgs a, uint32_t* status) {
    __shared__ uint32_t wave_tot[kTreePartNT / 64];
    __shared__ uint32_t s_sum[2];
    const uint32_t t = threadIdx.x;
    if (t < 2) s_sum[t] = 0;
    uint32_t carry = 0, n_e = 0, n_s = 0;
    for (uint32_t base = 0; base < n_parts; base += kTreePartNT) {
        const bool in = t < n_parts - base;
        const uint32_t v = in ? parts[base + t] : 0u;
        if (in) {
            n_e += parts[(size_t)n_parts + base + t];
            n_s += parts[2 * (size_t)n_parts + base + t];
        }
        uint32_t tot = 0;
        const uint32_t p = carry + block_exclusive_scan<kTreePartNT>(v, wave_tot, &tot);
        if (in) parts[base + t] = p;
        carry += tot;
    }
    __syncthreads();
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        n_e += (uint32_t)__shfl_xor((int)n_e, o);
        n_s += (uint32_t)__shfl_xor((int)n_s, o);
    }
    if ((t & 63u) == 0) {
        if (n_e) atomicAdd(&s_sum[0], n_e);  // (integer sums in LDS: the same on every run)
        if (n_s) atomicAdd(&s_sum[1], n_s);
    }
    __syncthreads();
    uint32_t err = 0;
    if (t == 0) {
        *a.n_out = carry;
        if (carry > a.out_max) err |= kErrCapacity;
        if (a.summary) {
            a.summary[0] = s_sum[0];
            a.summary[1] = s_sum[1];
            a.summary[2] = 0;
            a.summary[3] = 0;
            a.summary[4] = carry;
        }
    }
    flag_error(status, err);
}

__global__ __launch_bounds__(kTreeNT) void tree_diff_emit_kernel(TreeDiffArgs a, const uint32_t* parts) {
    __shared__ uint32_t s_cnt[kTreeSteps][kTreeNT / 64];
    const uint32_t t = threadIdx.x, w = t >> 6;
    uint32_t err = 0;  // (reported by tree_diff_count_kernel)
    const uint32_t n_list = tree_list_n(a.mine, err);
    uint32_t child[kTreeSteps], f[kTreeSteps];
    uint64_t b[kTreeSteps];
#pragma unroll
    for (int k = 0; k < kTreeSteps; ++k) {
        const uint32_t j = blockIdx.x * kTreeChunk + (uint32_t)k * kTreeRows + t / kDigTreeFanout;
        bool e, s;
        f[k] = tree_diff_flag(a, n_list, j, t & (kDigTreeFanout - 1), child[k], e, s, err);
        b[k] = ballot((f[k] & a.mask) != 0u);
        if ((t & 63u) == 0) s_cnt[k][w] = popc(b[k]);
    }
    __syncthreads();
    // the chunk's children in (step, wavefront, lane) order, which is (parent, slot) order
    uint32_t pos = parts[blockIdx.x];
#pragma unroll
    for (int k = 0; k < kTreeSteps; ++k) {
#pragma unroll
        for (int x = 0; x < kTreeNT / 64; ++x) {
            if ((uint32_t)x == w && (f[k] & a.mask) != 0u) {
                const uint32_t q = pos + below(b[k]);
                if (q < a.out_max) {  // nothing is written at or past out_max
                    a.idx_out[q] = child[k];
                    if (a.flags_out) a.flags_out[q] = (uint8_t)f[k];
                }
            }
            pos += s_cnt[k][x];
        }
    }
}

// parts: 3 words per chunk of kTreeChunk listed parents (digest_tree_diff_parts).
// n_max == 0: *n_out and the summary are still written.
size_t digest_tree_diff_parts(uint32_t n_max) { return 3 * (((size_t)n_max + kTreeChunk - 1) / kTreeChunk); }

hipError_t launch_digest_tree_diff(const uint64_t* mine_level, uint32_t n_level, const uint64_t* theirs,
                                   const uint32_t* parents, const uint32_t* n_parents, uint32_t n_max, uint32_t leaf,
                                   uint32_t mask, uint32_t* idx_out, uint8_t* flags_out, uint32_t* n_out,
                                   uint32_t out_max, uint32_t* summary, uint32_t* parts, uint32_t* status,
                                   hipStream_t stream) {
    const TreeDiffArgs a{TreeList{mine_level, n_level, parents, n_parents, n_max, aligned(mine_level, 16)},
                         theirs,
                         aligned(theirs, 16),
                         leaf,
                         mask,
                         idx_out,
                         flags_out,
                         n_out,
                         out_max,
                         summary};
    const uint32_t n_parts = (uint32_t)(((uint64_t)n_max + kTreeChunk - 1) / kTreeChunk);
    hipError_t e = hipSuccess;
    if (n_parts) {
        hipLaunchKernelGGL(tree_diff_count_kernel, dim3(n_parts), dim3(kTreeNT), 0, stream, a, parts, n_parts, status);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(tree_diff_partials_kernel, dim3(1), dim3(kTreePartNT), 0, stream, parts, n_parts, a, status);
    if ((e = hipGetLastError()) != hipSuccess || n_parts == 0) return e;
    hipLaunchKernelGGL(tree_diff_emit_kernel, dim3(n_parts), dim3(kTreeNT), 0, stream, a, parts);
    return hipGetLastError();
}

}  // namespace crdt
