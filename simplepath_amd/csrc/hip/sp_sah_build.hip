// sp_sah_build.hip -- binned SAH build on the device: the tree of
// sph::build_bvh_sah, byte for byte.
//
// Large nodes are split level by level.  One ids array stays stably partitioned; per level and
// open node: node and centroid bounds, 3 x 32 bins (count and box), one sweep and decision from
// sp_sah.h, a scan of the partition predicate and a scatter into the second ids array.  A range of
// at most `small` primitives is handed to one thread, which runs the host's recursion on it
// without a stack and numbers its nodes in pre-order as it goes.  Then the nodes the levels made
// get their subtree sizes bottom-up and pre-order indices top-down, and everything is written at
// its final index.
//
// Decision quantities are integer min / max / add atomics on order-mapped float bits (reduced in
// LDS first where a workgroup lies inside one node), which are deterministic.  A stored box is the
// host's fold over the node's slots in the order they have when the node is split: exact in a
// thread's recursion, and in the levels a min / max whose zero takes the sign of the last slot
// holding a zero (on a tie between +0 and -0 the fold keeps the later operand).  No launch reads bytes
// another workgroup wrote in that launch; the host reads three counters per level; no kernel spins.
#include "sp_sah_build.hpp"
#include "sp_devbuild.hpp"
#include "../common/sp_sah.h"

#include <type_traits>

namespace spb {
namespace {

static_assert(BLOCK == SAH_BLOCK, "the level kernels' workgroup");
constexpr uint32_t NONE    = 0xffffffffu;
constexpr uint32_t SUBREF  = 0x80000000u; // child reference: a handed-over range, not a level node
constexpr uint32_t NB      = 18;                 // words per open node: node box, centroid box, last zeros
constexpr uint32_t TBL     = 3 * 7 * sah::BINS;  // words of bins per open node: [axis][field][bin]
constexpr uint32_t MIN_ID  = 0xff800000u;        // fmap(+inf): identity of the mapped minimum
constexpr uint32_t MAX_ID  = 0x007fffffu;        // fmap(-inf): identity of the mapped maximum
constexpr uint32_t PARENT_MASK = (1u << 30) - 1u;

struct TopNode { // a node the level kernels split
    uint32_t first, count, left, right, axis, size, pre, height;
    float    lo[3], hi[3];
};
struct SubRoot { // a range one thread builds; its nodes lie at raw[2 * first ..) in local pre-order
    uint32_t first, count, size, height, pre;
};
struct Split { // one open node's decision
    uint32_t first, mid, last, moves; // moves: the predicate partitions the range (else the order stays)
    int      dim, bin;
    float    lo, k;
    uint32_t left_open, right_open;   // next level's open index of each child, NONE for a handed-over one
};
struct Counters {
    uint32_t next_open, tops, subs, bad; // bad: 1 a bound that is not finite, 2 an open node that did not split
};

// floats as unsigned integers of the same order
__device__ inline uint32_t fmap(float f)
{
    const uint32_t b = __float_as_uint(f);
    return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ inline float funmap(uint32_t u) { return __uint_as_float(u ^ ((u >> 31) ? 0x80000000u : 0xffffffffu)); }

// words of an open node's bounds: [0, 12) mapped lo3 / hi3 of the bounds and of the centroids;
// [12, 18) for each stored extreme the last slot that holds a zero there, (slot + 1) << 1 | sign
__device__ inline bool nb_is_min(uint32_t k) { return k < 12u && k % 6u < 3u; }
__device__ inline uint32_t nb_identity(uint32_t k) { return k >= 12u ? 0u : (k % 6u < 3u ? MIN_ID : MAX_ID); }

__device__ inline uint32_t tbl(int axis, int field, int bin) { return (uint32_t)((axis * 7 + field) * sah::BINS + bin); }

// Whether every slot of this workgroup lies in one open node (then *s0 is its index); returns
// false for all threads when no slot of it is open.  `s` is this thread's segment, NONE past n.
__device__ inline bool block_segment(uint32_t s, bool valid, bool& uniform, uint32_t& s0)
{
    __shared__ uint32_t first_seg;
    if (threadIdx.x == 0) first_seg = s;
    if (!__syncthreads_or(valid && s != NONE)) return false;
    s0      = first_seg;
    uniform = __syncthreads_and(!valid || s == s0) && s0 != NONE;
    return true;
}

__global__ __launch_bounds__(BLOCK) void sah_start(const sph::PrimBounds* __restrict__ bounds, uint32_t n, uint32_t root_open,
                                                   uint32_t* __restrict__ ids, uint32_t* __restrict__ seg,
                                                   Counters* __restrict__ cnt)
{
    const uint32_t i   = blockIdx.x * BLOCK + threadIdx.x;
    int            bad = 0;
    if (i < n) {
        ids[i] = i;
        seg[i] = root_open ? 0u : NONE;
        bad    = sah::finite_bounds(bounds[i].lo, bounds[i].hi) ? 0 : 1;
    }
    if (__syncthreads_or(bad) && threadIdx.x == 0) atomicOr(&cnt->bad, 1u);
}

__global__ __launch_bounds__(BLOCK) void sah_clear(uint32_t open, uint32_t* __restrict__ nb, uint32_t* __restrict__ bins)
{
    const uint64_t w = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (w < (uint64_t)open * NB) nb[w] = nb_identity((uint32_t)(w % NB));
    if (w < (uint64_t)open * TBL) {
        const uint32_t field = (uint32_t)(w % TBL) / sah::BINS % 7u;
        bins[w]              = field == 0u ? 0u : (field < 4u ? MIN_ID : MAX_ID);
    }
}

// Node box and centroid box of every open node.  The stored box is the host's fold over the node's
// slots in this level's order, where a tie between +0 and -0 goes to the later slot: the extreme
// itself is a min / max, and the sign of a zero extreme comes from the last slot that holds a zero.
__global__ __launch_bounds__(BLOCK) void sah_node_bounds(const sph::PrimBounds* __restrict__ bounds, const uint32_t* __restrict__ ids,
                                                         const uint32_t* __restrict__ seg, uint32_t n, uint32_t open,
                                                         uint32_t* __restrict__ nb)
{
    const uint32_t i     = blockIdx.x * BLOCK + threadIdx.x;
    const bool     valid = i < n;
    const uint32_t s     = valid ? seg[i] : NONE;
    bool           uniform = false;
    uint32_t       s0 = NONE;
    if (!block_segment(s, valid, uniform, s0)) return;
    uint32_t v[NB];
    for (uint32_t k = 0; k < NB; ++k) v[k] = nb_identity(k);
    if (s != NONE && s < open) {
        const sph::PrimBounds b = bounds[ids[i]];
        for (int d = 0; d < 3; ++d) {
            const uint32_t c = fmap(spm::centre(b.lo[d], b.hi[d]));
            v[d]     = fmap(b.lo[d]);
            v[3 + d] = fmap(b.hi[d]);
            v[6 + d] = c;
            v[9 + d] = c;
            if (b.lo[d] == 0.0f) v[12 + d] = (i + 1u) << 1 | __float_as_uint(b.lo[d]) >> 31;
            if (b.hi[d] == 0.0f) v[15 + d] = (i + 1u) << 1 | __float_as_uint(b.hi[d]) >> 31;
        }
    }
    if (uniform) { // one node: the waves reduce, LDS joins them, then one atomic per word and workgroup
        if (s0 >= open) return;
        __shared__ uint32_t red[NB];
        if (threadIdx.x < NB) red[threadIdx.x] = nb_identity(threadIdx.x);
        for (int o = 32; o > 0; o >>= 1)
            for (uint32_t k = 0; k < NB; ++k) {
                const uint32_t w = (uint32_t)__shfl_xor((int)v[k], o);
                v[k]             = nb_is_min(k) ? min(v[k], w) : max(v[k], w);
            }
        __syncthreads();
        if ((threadIdx.x & 63u) == 0u)
            for (uint32_t k = 0; k < NB; ++k) {
                if (nb_is_min(k)) atomicMin(&red[k], v[k]);
                else atomicMax(&red[k], v[k]);
            }
        __syncthreads();
        if (threadIdx.x < NB) {
            const uint32_t k = threadIdx.x, x = red[k];
            if (nb_is_min(k)) atomicMin(&nb[(size_t)s0 * NB + k], x);
            else if (x != nb_identity(k)) atomicMax(&nb[(size_t)s0 * NB + k], x);
        }
        return;
    }
    if (s == NONE || s >= open) return;
    for (uint32_t k = 0; k < NB; ++k) {
        if (nb_is_min(k)) atomicMin(&nb[(size_t)s * NB + k], v[k]);
        else if (v[k] != nb_identity(k)) atomicMax(&nb[(size_t)s * NB + k], v[k]);
    }
}

// one primitive into a bin table (LDS or global); cbw: the node's mapped centroid box
template <typename Table>
__device__ inline void add_to_bins(Table* t, const sph::PrimBounds& b, const uint32_t* __restrict__ cbw)
{
    uint32_t m[6];
    for (int e = 0; e < 3; ++e) {
        m[e]     = fmap(b.lo[e]);
        m[3 + e] = fmap(b.hi[e]);
    }
    for (int d = 0; d < 3; ++d) {
        const float lo = funmap(cbw[d]), hi = funmap(cbw[3 + d]);
        if (!(hi > lo)) continue;
        const int bi = sah::bin_of(spm::centre(b.lo[d], b.hi[d]), lo, sah::scale(lo, hi));
        atomicAdd(&t[tbl(d, 0, bi)], 1u);
        for (int e = 0; e < 3; ++e) {
            atomicMin(&t[tbl(d, 1 + e, bi)], m[e]);
            atomicMax(&t[tbl(d, 4 + e, bi)], m[3 + e]);
        }
    }
}

// counts and boxes of the 32 bins on each axis with extent.  A workgroup inside one node keeps the
// table in LDS (consecutive bins of a field lie in consecutive banks) and adds what it touched to
// the node's table; a workgroup across nodes goes to the tables directly.
__global__ __launch_bounds__(BLOCK) void sah_bins(const sph::PrimBounds* __restrict__ bounds, const uint32_t* __restrict__ ids,
                                                  const uint32_t* __restrict__ seg, uint32_t n, uint32_t open,
                                                  const uint32_t* __restrict__ nb, uint32_t* __restrict__ bins)
{
    __shared__ uint32_t tab[TBL];
    const uint32_t i     = blockIdx.x * BLOCK + threadIdx.x;
    const bool     valid = i < n;
    const uint32_t s     = valid ? seg[i] : NONE;
    bool           uniform = false;
    uint32_t       s0 = NONE;
    if (!block_segment(s, valid, uniform, s0)) return;
    if (uniform && s0 >= open) return;
    if (uniform) {
        for (uint32_t w = threadIdx.x; w < TBL; w += BLOCK) {
            const uint32_t field = w / sah::BINS % 7u;
            tab[w]               = field == 0u ? 0u : (field < 4u ? MIN_ID : MAX_ID);
        }
        __syncthreads();
    }
    if (s != NONE && s < open) {
        const sph::PrimBounds b = bounds[ids[i]];
        if (uniform) add_to_bins(tab, b, nb + (size_t)s * NB + 6);
        else add_to_bins(bins + (size_t)s * TBL, b, nb + (size_t)s * NB + 6);
    }
    if (!uniform) return;
    __syncthreads();
    uint32_t* g = bins + (size_t)s0 * TBL;
    for (uint32_t w = threadIdx.x; w < TBL; w += BLOCK) {
        const uint32_t field = w / sah::BINS % 7u, x = tab[w];
        if (field == 0u) {
            if (x) atomicAdd(&g[w], x);
        } else if (field < 4u) {
            if (x != MIN_ID) atomicMin(&g[w], x);
        } else if (x != MAX_ID) atomicMax(&g[w], x);
    }
}

// One thread per open node: the sweeps and the decision, the split position from the bin counts,
// and the two children -- a larger one opens at the next level, a small one is handed over.
// Indices come from counters; their order does not reach the tree, which is numbered afterwards.
__global__ __launch_bounds__(64) void sah_decide(uint32_t open, const uint32_t* __restrict__ open_top, const uint32_t* __restrict__ nb,
                                                 const uint32_t* __restrict__ bins, uint32_t max_leaf, uint32_t small,
                                                 uint32_t top_cap, uint32_t sub_cap, uint32_t open_cap, TopNode* __restrict__ tops,
                                                 SubRoot* __restrict__ subs, Split* __restrict__ split,
                                                 uint32_t* __restrict__ open_top_next, Counters* __restrict__ cnt)
{
    const uint32_t j = blockIdx.x * 64u + threadIdx.x;
    if (j >= open) return;
    const uint32_t  me = open_top[j];
    const uint32_t* w  = nb + (size_t)j * NB;
    sah::Box        bb, cb;
    for (int d = 0; d < 3; ++d) {
        bb.lo[d] = funmap(w[d]);
        bb.hi[d] = funmap(w[3 + d]);
        cb.lo[d] = funmap(w[6 + d]);
        cb.hi[d] = funmap(w[9 + d]);
        if (bb.lo[d] == 0.0f) bb.lo[d] = __uint_as_float(w[12 + d] << 31);
        if (bb.hi[d] == 0.0f) bb.hi[d] = __uint_as_float(w[15 + d] << 31);
    }
    const uint32_t  first = tops[me].first, count = tops[me].count, last = first + count;
    const uint32_t* t = bins + (size_t)j * TBL;
    sah::Best       best;
    for (int d = 0; d < 3; ++d) {
        if (!(cb.hi[d] > cb.lo[d])) continue;
        sah::Box bx[sah::BINS];
        int      c[sah::BINS];
        for (int b = 0; b < sah::BINS; ++b) {
            c[b]  = (int)t[tbl(d, 0, b)];
            bx[b] = sah::empty_box();
            if (c[b])
                for (int e = 0; e < 3; ++e) {
                    bx[b].lo[e] = funmap(t[tbl(d, 1 + e, b)]);
                    bx[b].hi[e] = funmap(t[tbl(d, 4 + e, b)]);
                }
        }
        sah::sweep(d, c, bx, best);
    }
    const sah::Decision what = sah::decide(bb, count, max_leaf, best);
    Split               sp{};
    sp.first = first;
    sp.last  = last;
    sp.mid   = first + count / 2u;
    sp.left_open = sp.right_open = NONE;
    if (what == sah::LEAF) { // (count > small >= max_leaf: cannot happen)
        atomicOr(&cnt->bad, 2u);
        sp.mid   = last;
        split[j] = sp;
        return;
    }
    uint32_t axis = 0;
    if (what == sah::SPLIT) {
        uint32_t lefts = 0;
        for (int b = 0; b <= best.bin; ++b) lefts += t[tbl(best.dim, 0, b)];
        axis   = (uint32_t)best.dim;
        sp.dim = best.dim;
        sp.bin = best.bin;
        sp.lo  = cb.lo[best.dim];
        sp.k   = sah::scale(cb.lo[best.dim], cb.hi[best.dim]);
        if (lefts != 0u && lefts != count) { // (else: the order stays, halved by index)
            sp.moves = 1u;
            sp.mid   = first + lefts;
        }
    }
    uint32_t ref[2];
    for (int side = 0; side < 2; ++side) {
        const uint32_t f = side ? sp.mid : first, c = side ? last - sp.mid : sp.mid - first;
        if (c > small) {
            const uint32_t o = atomicAdd(&cnt->next_open, 1u), ti = atomicAdd(&cnt->tops, 1u);
            ref[side] = ti;
            if (ti < top_cap && o < open_cap) {
                TopNode tn{};
                tn.first = f;
                tn.count = c;
                tops[ti] = tn;
                open_top_next[o]                    = ti;
                (side ? sp.right_open : sp.left_open) = o;
            }
        } else {
            const uint32_t si = atomicAdd(&cnt->subs, 1u);
            ref[side] = si | SUBREF;
            if (si < sub_cap) subs[si] = SubRoot{ f, c, 0u, 0u, 0u };
        }
    }
    for (int d = 0; d < 3; ++d) {
        tops[me].lo[d] = bb.lo[d];
        tops[me].hi[d] = bb.hi[d];
    }
    tops[me].left  = ref[0];
    tops[me].right = ref[1];
    tops[me].axis  = axis;
    split[j]       = sp;
}

__global__ __launch_bounds__(BLOCK) void sah_flags(const sph::PrimBounds* __restrict__ bounds, const uint32_t* __restrict__ ids,
                                                   const uint32_t* __restrict__ seg, uint32_t n, uint32_t open,
                                                   const Split* __restrict__ split, uint32_t* __restrict__ flag)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t s = seg[i];
    uint32_t       f = 0;
    if (s != NONE && s < open && split[s].moves) {
        const Split           sp = split[s];
        const sph::PrimBounds b  = bounds[ids[i]];
        f = sah::goes_left(spm::centre(b.lo[sp.dim], b.hi[sp.dim]), sp.lo, sp.k, sp.bin) ? 1u : 0u;
    }
    flag[i] = f;
}

// `rank` is the exclusive scan of `flag` over all slots: within a node, rank[i] - rank[first] lefts precede slot i
__global__ __launch_bounds__(BLOCK) void sah_scatter(const uint32_t* __restrict__ ids, const uint32_t* __restrict__ seg, uint32_t n,
                                                     uint32_t open, const Split* __restrict__ split,
                                                     const uint32_t* __restrict__ flag, const uint32_t* __restrict__ rank,
                                                     uint32_t* __restrict__ ids_next, uint32_t* __restrict__ seg_next)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t s = seg[i];
    uint32_t       dest = i, to = NONE;
    if (s != NONE && s < open) {
        const Split sp = split[s];
        if (sp.moves) {
            const uint32_t lefts = rank[i] - rank[sp.first];
            dest                 = flag[i] ? sp.first + lefts : sp.mid + (i - sp.first - lefts);
        }
        if (dest < sp.first || dest >= sp.last) dest = i; // (cannot happen: the counts and the scan agree)
        to = dest < sp.mid ? sp.left_open : sp.right_open;
    }
    ids_next[dest] = ids[i];
    seg_next[dest] = to;
}

// One thread per handed-over range: SahBuilder::build on it, depth first, without a stack.  Local
// node x lies at raw[2 * first + x]; the left child of x is x + 1, so the local index is the
// pre-order offset.  While a node's left subtree is built, its a / b hold first / mid and `up`
// holds parent | axis << 30 and last; a finished inner node has a = left | axis << 30, b = right.
__global__ __launch_bounds__(64) void sah_subtrees(const sph::PrimBounds* __restrict__ bounds, uint32_t* __restrict__ ids,
                                                   uint32_t* __restrict__ tmp, SubRoot* __restrict__ subs, uint32_t n_subs,
                                                   uint32_t max_leaf, Node* __restrict__ raw, uint2* __restrict__ up)
{
    const uint32_t s = blockIdx.x * 64u + threadIdx.x;
    if (s >= n_subs) return;
    const uint32_t f0 = subs[s].first, cap = 2u * subs[s].count;
    Node*          R = raw + 2 * (size_t)f0;
    uint2*         U = up + 2 * (size_t)f0;
    uint32_t       cur = 0, f = f0, l = f0 + subs[s].count, parent = PARENT_MASK;
    uint32_t       depth = 0, height = 0;
    for (;;) {
        if (cur >= cap) break; // (cannot happen: c primitives make at most 2c - 1 nodes)
        const uint32_t x = cur++;
        height           = max(height, ++depth);
        sah::Box bb = sah::empty_box(), cb = sah::empty_box();
        for (uint32_t i = f; i < l; ++i) {
            const sph::PrimBounds b = bounds[ids[i]];
            float                 c[3];
            for (int d = 0; d < 3; ++d) c[d] = spm::centre(b.lo[d], b.hi[d]);
            spm::fold(bb, b.lo, b.hi);
            spm::fold(cb, c, c);
        }
        const uint32_t n    = l - f;
        sah::Decision  what = sah::LEAF;
        sah::Best      best;
        if (n > 1u) {
            for (int d = 0; d < 3; ++d) {
                const float lo = cb.lo[d], hi = cb.hi[d];
                if (!(hi > lo)) continue;
                const float k = sah::scale(lo, hi);
                sah::Box    bx[sah::BINS];
                int         c[sah::BINS];
                for (int b = 0; b < sah::BINS; ++b) {
                    bx[b] = sah::empty_box();
                    c[b]  = 0;
                }
                for (uint32_t i = f; i < l; ++i) {
                    const sph::PrimBounds b  = bounds[ids[i]];
                    const int             bi = sah::bin_of(spm::centre(b.lo[d], b.hi[d]), lo, k);
                    c[bi]++;
                    spm::fold(bx[bi], b.lo, b.hi);
                }
                sah::sweep(d, c, bx, best);
            }
            what = sah::decide(bb, n, max_leaf, best);
        }
        Node nd;
        for (int d = 0; d < 3; ++d) {
            nd.lo[d] = bb.lo[d];
            nd.hi[d] = bb.hi[d];
        }
        if (what != sah::LEAF) {
            uint32_t mid = f + n / 2u, axis = 0;
            if (what == sah::SPLIT) {
                const float lo = cb.lo[best.dim], k = sah::scale(cb.lo[best.dim], cb.hi[best.dim]);
                axis           = (uint32_t)best.dim;
                uint32_t to    = f;
                for (uint32_t i = f; i < l; ++i) {
                    const sph::PrimBounds b = bounds[ids[i]];
                    if (sah::goes_left(spm::centre(b.lo[best.dim], b.hi[best.dim]), lo, k, best.bin)) tmp[to++] = ids[i];
                }
                if (to != f && to != l) {
                    mid = to;
                    for (uint32_t i = f; i < l; ++i) {
                        const sph::PrimBounds b = bounds[ids[i]];
                        if (!sah::goes_left(spm::centre(b.lo[best.dim], b.hi[best.dim]), lo, k, best.bin)) tmp[to++] = ids[i];
                    }
                    for (uint32_t i = f; i < l; ++i) ids[i] = tmp[i];
                }
            }
            nd.a   = f;
            nd.b   = mid;
            R[x]   = nd;
            U[x]   = make_uint2(parent | axis << 30, l);
            parent = x;
            l      = mid;
            continue;
        }
        nd.a = f;
        nd.b = n | sph::BVH_LEAF;
        R[x] = nd;
        U[x] = make_uint2(parent, l);
        // up, until a node whose right child is still to build
        uint32_t c    = x;
        bool     done = false;
        for (;;) {
            --depth;
            if (c == 0u) {
                done = true;
                break;
            }
            const uint32_t p = U[c].x & PARENT_MASK;
            if (c == p + 1u) {
                const uint2 u = U[p];
                f             = R[p].b;
                l             = u.y;
                R[p].a        = (p + 1u) | (u.x >> 30) << sph::BVH_AXIS_SHIFT;
                R[p].b        = cur;
                parent        = p;
                break;
            }
            c = p;
        }
        if (done) break;
    }
    subs[s].size   = cur;
    subs[s].height = height;
}

// bottom-up over one level of the nodes the level kernels made: size and height from the children
__global__ __launch_bounds__(64) void sah_sum_level(TopNode* __restrict__ tops, uint32_t begin, uint32_t end,
                                                    const SubRoot* __restrict__ subs)
{
    const uint32_t t = begin + blockIdx.x * 64u + threadIdx.x;
    if (t >= end) return;
    uint32_t size = 1, height = 0;
    for (int side = 0; side < 2; ++side) {
        const uint32_t r = side ? tops[t].right : tops[t].left;
        size += (r & SUBREF) ? subs[r & ~SUBREF].size : tops[r].size;
        height = max(height, (r & SUBREF) ? subs[r & ~SUBREF].height : tops[r].height);
    }
    tops[t].size   = size;
    tops[t].height = height + 1u;
}

// top-down: left = me + 1, right = me + 1 + nodes(left)
__global__ __launch_bounds__(64) void sah_number_level(TopNode* __restrict__ tops, uint32_t begin, uint32_t end,
                                                       SubRoot* __restrict__ subs)
{
    const uint32_t t = begin + blockIdx.x * 64u + threadIdx.x;
    if (t >= end) return;
    const uint32_t l = tops[t].left, r = tops[t].right, pl = tops[t].pre + 1u;
    const uint32_t pr = pl + ((l & SUBREF) ? subs[l & ~SUBREF].size : tops[l].size);
    if (l & SUBREF) subs[l & ~SUBREF].pre = pl;
    else tops[l].pre = pl;
    if (r & SUBREF) subs[r & ~SUBREF].pre = pr;
    else tops[r].pre = pr;
}

__global__ __launch_bounds__(64) void sah_emit_tops(const TopNode* __restrict__ tops, uint32_t n_tops, const SubRoot* __restrict__ subs,
                                                    uint32_t m, Node* __restrict__ nodes)
{
    const uint32_t t = blockIdx.x * 64u + threadIdx.x;
    if (t >= n_tops) return;
    const TopNode& tn = tops[t];
    if (tn.pre >= m) return;
    Node nd;
    for (int d = 0; d < 3; ++d) {
        nd.lo[d] = tn.lo[d];
        nd.hi[d] = tn.hi[d];
    }
    nd.a = ((tn.left & SUBREF) ? subs[tn.left & ~SUBREF].pre : tops[tn.left].pre) | tn.axis << sph::BVH_AXIS_SHIFT;
    nd.b = (tn.right & SUBREF) ? subs[tn.right & ~SUBREF].pre : tops[tn.right].pre;
    nodes[tn.pre] = nd;
}

// one wave per handed-over range: its nodes move to pre + local index, child links with them
__global__ __launch_bounds__(64) void sah_emit_subtrees(const SubRoot* __restrict__ subs, uint32_t n_subs, const Node* __restrict__ raw,
                                                        uint32_t m, Node* __restrict__ nodes)
{
    if (blockIdx.x >= n_subs) return;
    const SubRoot s = subs[blockIdx.x];
    const Node*   R = raw + 2 * (size_t)s.first;
    for (uint32_t x = threadIdx.x; x < s.size; x += 64u) {
        if (s.pre + x >= m) return;
        Node nd = R[x];
        if (!(nd.b & sph::BVH_LEAF)) {
            nd.a += s.pre; // (the axis bits stay: indices are below 2^30)
            nd.b += s.pre;
        }
        nodes[s.pre + x] = nd;
    }
}

} // namespace

int build_sah_device(const std::vector<sph::PrimBounds>& bounds, int max_leaf, sph::Bvh& out, SahStats& st, std::string& err,
                     bool timed, DeviceTree* keep, uint32_t small)
{
    st             = SahStats{};
    const size_t n = bounds.size();
    open_binary(n, max_leaf, "SAH BVH", out, keep);
    if (n <= 1) { // empty, or one leaf
        out = sph::build_bvh_sah_levels(bounds, max_leaf);
        return SP_OK;
    }
    small = small ? std::min(std::max(small, SAH_SMALL_MIN), SAH_SMALL_MAX) : SAH_SMALL_DEFAULT;
    Stage  stage("device SAH build", err, timed);
    Arena& mem = stage.mem; // (the name the error texts carry)

    const uint32_t un = (uint32_t)n;
    // every open node holds more than `small` slots, and the open nodes of a level are disjoint
    const uint32_t open_cap = un / (small + 1u) + 1u;
    sph::PrimBounds* d_bounds = nullptr;
    uint32_t *       d_ids[2] = { nullptr, nullptr }, *d_seg[2] = { nullptr, nullptr }, *d_flag = nullptr, *d_rank = nullptr;
    uint32_t *       d_open[2] = { nullptr, nullptr }, *d_nb = nullptr, *d_bins = nullptr;
    Split*           d_split = nullptr;
    Counters*        d_cnt = nullptr;
    SPB_HIP(mem.get(&d_bounds, n));
    for (int k = 0; k < 2; ++k) {
        SPB_HIP(mem.get(&d_ids[k], n));
        SPB_HIP(mem.get(&d_seg[k], n));
        SPB_HIP(mem.get(&d_open[k], open_cap));
    }
    SPB_HIP(mem.get(&d_flag, n));
    SPB_HIP(mem.get(&d_rank, n));
    SPB_HIP(mem.get(&d_nb, (size_t)open_cap * NB));
    SPB_HIP(mem.get(&d_bins, (size_t)open_cap * TBL));
    SPB_HIP(mem.get(&d_split, open_cap));
    SPB_HIP(mem.get(&d_cnt, 1));
    Scan scan;
    SPB_HIP(scan.reserve(mem, n));
    SPB_HIP(hipMemcpy(d_bounds, bounds.data(), n * sizeof(sph::PrimBounds), hipMemcpyHostToDevice));
    stage.lap(st.ms_bounds_up);

    // the nodes the levels make and the handed-over ranges: both grow with the tree
    TopNode* d_tops = nullptr;
    SubRoot* d_subs = nullptr;
    uint32_t top_cap = 0, sub_cap = 0;
    auto     reserve = [&](auto*& ptr, uint32_t& cap, uint32_t used, uint32_t want) -> hipError_t {
        if (want <= cap) return hipSuccess;
        using T           = std::remove_reference_t<decltype(*ptr)>;
        const uint32_t nc = std::max(want, cap * 2u);
        T*             np = nullptr;
        hipError_t     e  = mem.get(&np, nc);
        if (e != hipSuccess) return e;
        if (used) e = hipMemcpy(np, ptr, (size_t)used * sizeof(T), hipMemcpyDeviceToDevice);
        if (ptr) mem.drop(ptr);
        ptr = np;
        cap = nc;
        return e;
    };
    const bool root_open = un > small;
    Counters   c{};
    c.tops = root_open ? 1u : 0u;
    c.subs = root_open ? 0u : 1u;
    SPB_HIP(reserve(d_tops, top_cap, 0u, 64u));
    SPB_HIP(reserve(d_subs, sub_cap, 0u, 64u));
    SPB_HIP(hipMemcpy(d_cnt, &c, sizeof c, hipMemcpyHostToDevice));
    if (root_open) {
        TopNode root{};
        root.count = un;
        const uint32_t zero = 0;
        SPB_HIP(hipMemcpy(d_tops, &root, sizeof root, hipMemcpyHostToDevice));
        SPB_HIP(hipMemcpy(d_open[0], &zero, 4, hipMemcpyHostToDevice));
    } else {
        const SubRoot root{ 0u, un, 0u, 0u, 0u };
        SPB_HIP(hipMemcpy(d_subs, &root, sizeof root, hipMemcpyHostToDevice));
    }
    hipLaunchKernelGGL(sah_start, dim3(blocks_for(n)), dim3(BLOCK), 0, 0, d_bounds, un, root_open ? 1u : 0u, d_ids[0], d_seg[0], d_cnt);
    SPB_HIP(hipGetLastError());
    SPB_HIP(hipMemcpy(&c, d_cnt, sizeof c, hipMemcpyDeviceToHost));
    if (c.bad & 1u) return stage.refuse("a primitive's bounds are not finite", SP_ERR_UNSUPPORTED);

    // ---- the levels
    std::vector<uint32_t> level_begin; // of the level nodes, by level; the last entry is their count
    uint32_t              open = root_open ? 1u : 0u;
    int                   cur  = 0;
    level_begin.push_back(0u);
    while (open) {
        level_begin.push_back(c.tops);
        if (open > open_cap) return stage.refuse("more open nodes than slots allow");
        SPB_HIP(reserve(d_tops, top_cap, c.tops, c.tops + 2u * open));
        SPB_HIP(reserve(d_subs, sub_cap, c.subs, c.subs + 2u * open));
        SPB_HIP(hipMemsetAsync(&d_cnt->next_open, 0, 4, hipStream_t(0)));
        hipLaunchKernelGGL(sah_clear, dim3(blocks_for((uint64_t)open * TBL)), dim3(BLOCK), 0, 0, open, d_nb, d_bins);
        hipLaunchKernelGGL(sah_node_bounds, dim3(blocks_for(n)), dim3(BLOCK), 0, 0, d_bounds, d_ids[cur], d_seg[cur], un, open, d_nb);
        hipLaunchKernelGGL(sah_bins, dim3(blocks_for(n)), dim3(BLOCK), 0, 0, d_bounds, d_ids[cur], d_seg[cur], un, open, d_nb, d_bins);
        hipLaunchKernelGGL(sah_decide, dim3(blocks_for(open, 64)), dim3(64), 0, 0, open, d_open[cur], d_nb, d_bins, (uint32_t)max_leaf,
                           small, top_cap, sub_cap, open_cap, d_tops, d_subs, d_split, d_open[cur ^ 1], d_cnt);
        hipLaunchKernelGGL(sah_flags, dim3(blocks_for(n)), dim3(BLOCK), 0, 0, d_bounds, d_ids[cur], d_seg[cur], un, open, d_split, d_flag);
        SPB_HIP(hipGetLastError());
        SPB_HIP(scan.run(d_flag, d_rank, n));
        hipLaunchKernelGGL(sah_scatter, dim3(blocks_for(n)), dim3(BLOCK), 0, 0, d_ids[cur], d_seg[cur], un, open, d_split, d_flag, d_rank,
                           d_ids[cur ^ 1], d_seg[cur ^ 1]);
        SPB_HIP(hipGetLastError());
        const uint32_t tops_before = c.tops, subs_before = c.subs;
        SPB_HIP(hipMemcpy(&c, d_cnt, sizeof c, hipMemcpyDeviceToHost));
        ++st.levels;
        if ((c.bad & 2u) || c.tops + c.subs != tops_before + subs_before + 2u * open || c.tops > top_cap || c.subs > sub_cap ||
            c.next_open != c.tops - tops_before)
            return stage.refuse("a level did not split every open node");
        open = c.next_open;
        cur ^= 1;
    }
    level_begin.push_back(c.tops); // level k of the level nodes: [level_begin[k], level_begin[k + 1])
    stage.lap(st.ms_levels);
    // the level scratch goes before the nodes come
    const uint32_t n_tops = c.tops, n_subs = c.subs;
    st.top_nodes = n_tops;
    st.subtrees  = n_subs;
    uint32_t* d_order = d_ids[cur];
    uint32_t* d_tmp   = d_ids[cur ^ 1];
    for (uint32_t* p : { d_seg[0], d_seg[1], d_flag, d_rank, d_bins }) mem.drop(p);

    // ---- the handed-over ranges
    Node*  d_raw = nullptr;
    uint2* d_up  = nullptr;
    SPB_HIP(mem.get(&d_raw, 2 * n));
    SPB_HIP(mem.get(&d_up, 2 * n));
    hipLaunchKernelGGL(sah_subtrees, dim3(blocks_for(n_subs, 64)), dim3(64), 0, 0, d_bounds, d_order, d_tmp, d_subs, n_subs,
                       (uint32_t)max_leaf, d_raw, d_up);
    SPB_HIP(hipGetLastError());
    stage.lap(st.ms_subtrees);

    // ---- sizes bottom-up, pre-order indices top-down
    const size_t n_levels = level_begin.size() - 1; // the first and the last "level" may be empty
    for (size_t k = n_levels; k-- > 0;) {
        const uint32_t b = level_begin[k], e = level_begin[k + 1];
        if (e > b) hipLaunchKernelGGL(sah_sum_level, dim3(blocks_for(e - b, 64)), dim3(64), 0, 0, d_tops, b, e, d_subs);
    }
    for (size_t k = 0; k < n_levels; ++k) {
        const uint32_t b = level_begin[k], e = level_begin[k + 1];
        if (e > b) hipLaunchKernelGGL(sah_number_level, dim3(blocks_for(e - b, 64)), dim3(64), 0, 0, d_tops, b, e, d_subs);
    }
    SPB_HIP(hipGetLastError());
    uint32_t m = 0, height = 0;
    if (root_open) {
        TopNode root{};
        SPB_HIP(hipMemcpy(&root, d_tops, sizeof root, hipMemcpyDeviceToHost));
        m      = root.size;
        height = root.height;
    } else {
        SubRoot root{};
        SPB_HIP(hipMemcpy(&root, d_subs, sizeof root, hipMemcpyDeviceToHost));
        m      = root.size;
        height = root.height;
    }
    if (m == 0 || m > 2u * un - 1u) return stage.refuse("the node count is out of range");
    stage.lap(st.ms_number);

    // ---- every node at its final index
    Node* d_nodes = nullptr;
    SPB_HIP(mem.get(&d_nodes, m));
    if (n_tops) hipLaunchKernelGGL(sah_emit_tops, dim3(blocks_for(n_tops, 64)), dim3(64), 0, 0, d_tops, n_tops, d_subs, m, d_nodes);
    hipLaunchKernelGGL(sah_emit_subtrees, dim3(n_subs), dim3(64), 0, 0, d_subs, n_subs, d_raw, m, d_nodes);
    SPB_HIP(hipGetLastError());
    SPB_HIP(hipDeviceSynchronize());
    stage.lap(st.ms_emit);
    st.peak_bytes = mem.peak;
    out.max_depth = (int)height;
    return finish_binary(stage, d_nodes, m, d_order, un, keep, out, st.ms_copy_back);
}

} // namespace spb
