// gf_locate.hip — names the one silently corrupted shard of an object from
// the syndromes the fused decode already computes (gf_locate.h).
//
// gf_locate<X>: one workgroup = 256 lanes x one 16-B vector of one object,
// launch policy as the check-only passes of gf_kernels.hip (nt loads, XCD-
// contiguous order, full occupancy).  The k survivor rows stream through a
// runtime loop, four loads in flight per lane; the inputs are not kept: the
// candidate tests need only the X syndromes and the tables of C the pass
// carries.  Clean data takes one wave-uniform branch per vector and no more.
// gf_locate_finish: one lane per object turns the OR-ed scratch word into the
// result and zeroes the word for the next call.
// gf_locate_masked / gf_locate_finish_masked / gf_locate_lanes: the same for a
// batch whose objects each bring their own present mask (second half).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "gf_device.h"
#include "gf_launch.h"
#include "gf_locate.h"
#include "gf_masked.h"

namespace rsgpu {

namespace {

template <int X>
struct LocArgs {
    const uint8_t *base;
    uint64_t obj_stride;
    uint32_t *acc;   // per object: dead positions | kLocSeen (atomicOr)
    uint32_t nvec;   // 16-B vectors per row
    uint32_t tail;   // valid bytes in the last vector (1..16)
    uint32_t span;   // bytes addressable from an object base
    uint32_t pitch;
    uint32_t K;      // survivors (k)
    uint64_t order;  // nibble q: the shard at column position q (S then E)
    Order ord;
    uint32_t tab[(kLocMaxN - X) * X * kTabWords];  // [c][r]: table of C[r][c]
};

// c (x) w for one dword
template <typename T>
__device__ __forceinline__ uint32_t gf_mulc(T *t, const GfIdx &g) {
    return gf_mac(0u, t, g);
}

template <int X, int BS, int LAUX>
__global__ __launch_bounds__(BS) void gf_locate(const LocArgs<X> a) {
    uint32_t obj, chunk;
    if (!wg_item(a.ord, obj, chunk)) return;
    // no lane leaves early: the ballots below count every lane of the wave
    const uint32_t v = chunk * BS + threadIdx.x;
    const bool act = v < a.nvec;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
        (void *)(a.base + (uint64_t)obj * a.obj_stride), (short)0, (int)a.span, 0x00020000);
    const uint32_t K = a.K;
    auto row_off = [&](uint32_t q) -> uint32_t { return ((uint32_t)(a.order >> (4u * q)) & 15u) * a.pitch; };

    uint32_t s[X][4];
#pragma unroll
    for (int r = 0; r < X; ++r)
#pragma unroll
        for (int d = 0; d < 4; ++d) s[r][d] = 0;

    // survivors: s[r] ^= C[r][c] (x) row c, four rows' loads issued together
    for (uint32_t c0 = 0; c0 < K; c0 += 4) {
        u32x4 x[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            x[j] = u32x4{0u, 0u, 0u, 0u};
            if (act && c0 + j < K) x[j] = __builtin_amdgcn_raw_buffer_load_b128(rs, v * 16u, row_off(c0 + j), LAUX);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (c0 + j < K) {
#pragma unroll
                for (int d = 0; d < 4; ++d) {
                    const GfIdx g = gf_idx(x[j][d]);
#pragma unroll
                    for (int r = 0; r < X; ++r) s[r][d] = gf_mac(s[r][d], &a.tab[((c0 + j) * X + r) * kTabWords], g);
                }
            }
        }
    }
    // extras: identity inputs, row K + t enters syndrome t only
    {
        u32x4 x[X];
#pragma unroll
        for (int t = 0; t < X; ++t) {
            x[t] = u32x4{0u, 0u, 0u, 0u};
            if (act) x[t] = __builtin_amdgcn_raw_buffer_load_b128(rs, v * 16u, row_off(K + t), LAUX);
        }
#pragma unroll
        for (int t = 0; t < X; ++t)
#pragma unroll
            for (int d = 0; d < 4; ++d) s[t][d] ^= x[t][d];
    }
    // bytes past shard_len (row padding) take no part
    const uint32_t valid = (v == a.nvec - 1) ? a.tail : 16u;
    uint32_t any = 0;
#pragma unroll
    for (int r = 0; r < X; ++r)
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            s[r][d] &= tail_mask(d, valid);
            any |= s[r][d];
        }
    if (__builtin_amdgcn_ballot_w64(any != 0) == 0) return;  // wave-uniform: clean vectors end here

    // Candidate tests.  Column position q is dead when some byte column's
    // syndromes are not parallel to column q of H = [C | I]:
    // H[b][q] (x) s_a != H[a][q] (x) s_b for a row pair a < b.  Lanes with
    // zero syndromes pass every test (0 == 0) and set nothing.
    uint32_t m = 0;
    if (any != 0) {
        m = kLocSeen;
        GfIdx g[X][4];
#pragma unroll
        for (int r = 0; r < X; ++r)
#pragma unroll
            for (int d = 0; d < 4; ++d) g[r][d] = gf_idx(s[r][d]);
        for (uint32_t q = 0; q < K; ++q) {  // survivor positions: column q of C
            uint32_t diff = 0;
#pragma unroll
            for (int ra = 0; ra < X; ++ra)
#pragma unroll
                for (int rb = ra + 1; rb < X; ++rb)
#pragma unroll
                    for (int d = 0; d < 4; ++d)
                        diff |= gf_mulc(&a.tab[(q * X + rb) * kTabWords], g[ra][d]) ^
                                gf_mulc(&a.tab[(q * X + ra) * kTabWords], g[rb][d]);
            if (diff) m |= 1u << q;
        }
        // extra position K + t: column e_t, dead when any other syndrome is non-zero
        uint32_t nzr[X];
#pragma unroll
        for (int r = 0; r < X; ++r) nzr[r] = s[r][0] | s[r][1] | s[r][2] | s[r][3];
#pragma unroll
        for (int t = 0; t < X; ++t) {
            uint32_t other = 0;
#pragma unroll
            for (int r = 0; r < X; ++r)
                if (r != t) other |= nzr[r];
            if (other) m |= 1u << (K + t);
        }
    }
    // OR across the wave (one ballot per mask bit: scalar results), then one
    // device-scope atomic per wave; OR is order-independent
    uint32_t wm = 0;
#pragma unroll
    for (int i = 0; i <= 16; ++i)
        if (__builtin_amdgcn_ballot_w64(((m >> i) & 1u) != 0) != 0) wm |= 1u << i;
    if ((threadIdx.x & 63u) == 0) atomicOr(&a.acc[obj], wm);
}

// zeroes the words the locate kernel ORs into, when they are not the ring's
// (launch_zero_u32)
__global__ __launch_bounds__(256) void gf_locate_clear(uint32_t *acc, uint32_t nobj) {
    const uint32_t o = blockIdx.x * 256u + threadIdx.x;
    if (o < nobj) acc[o] = 0u;
}

__global__ __launch_bounds__(256) void gf_locate_finish(uint32_t *acc, uint32_t nobj, uint32_t npos, uint64_t order,
                                                        uint32_t present, int32_t *loc, uint32_t *masks) {
    const uint32_t o = blockIdx.x * 256u + threadIdx.x;
    if (o >= nobj) return;
    const uint32_t w = acc[o];
    // the scratch is left zero; acc may be loc itself (a captured call,
    // rsgpu.cpp run_locate): the word is then overwritten with the result
    if (w && (const void *)acc != (const void *)loc) acc[o] = 0u;
    int32_t r = kLocClean;
    uint32_t mask = present;
    if (w) {
        const uint32_t alive = ~w & ((1u << npos) - 1u);
        r = kLocUnlocatable;
        if (__builtin_popcount(alive) == 1) {
            r = (int32_t)((order >> (4u * (uint32_t)__builtin_ctz(alive))) & 15u);
            mask &= ~(1u << r);
        }
    }
    loc[o] = r;
    if (masks) masks[o] = mask;
}

template <int X>
hipError_t launch_locate_t(const LocPlan &P, const Layout &L, uint32_t *acc, uint64_t order, hipStream_t st) {
    LocArgs<X> a{};
    a.obj_stride = L.obj_stride;
    a.nvec = (uint32_t)((L.shard_len + 15) / 16);
    a.tail = (uint32_t)(L.shard_len - (size_t)(a.nvec - 1) * 16);
    a.pitch = (uint32_t)L.pitch;
    // every row of the code is addressable (the launch reads the present ones)
    a.span = (uint32_t)((size_t)(P.nrows - 1) * L.pitch + (size_t)a.nvec * 16);
    a.K = (uint32_t)P.K;
    a.order = order;
    std::memcpy(a.tab, P.tab, sizeof(uint32_t) * (size_t)P.K * X * kTabWords);
    const unsigned gx = (a.nvec + kBlock - 1) / kBlock;
    const int step = max_items(gx);
    for (int o0 = 0; o0 < L.nobj; o0 += step) {
        const int no = std::min(step, L.nobj - o0);
        a.base = L.base + (size_t)o0 * L.obj_stride;
        a.acc = acc + o0;
        unsigned grid;
        a.ord = make_order(gx, (uint32_t)no, objs_span(L, no, a.span), grid);
        hipLaunchKernelGGL((gf_locate<X, kBlock, kLoadAux>), dim3(grid), dim3(kBlock), 0, st, a);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// ------------------------------------------------ per-object patterns
// rsgpu_locate_dev_masks: every object brings its own present mask.

struct LocMArgs {  // long rows: gf_locate_masked
    const uint8_t *base;
    uint64_t obj_stride;
    const uint32_t *present;  // [nobj] present bitmasks
    const int32_t *pat;       // [1 << n]: slot or kLocTooFew / TooMany / Singular
    const LocRec *recs;       // [slot]
    const uint32_t *tabs;     // [slot][K][XM][kTabWords]
    uint32_t *acc;            // as LocArgs::acc
    uint32_t nmask;           // (1 << n) - 1
    uint32_t K, XM;           // survivors; rows of a slot's tables
    uint32_t nvec, tail, span, pitch;
    Order ord;
};

// gf_locate's body for one object whose order and tables come from its atlas
// record (constant address space: scalar loads).  PAD: the code's largest X
// for every object; an object with xobj < X extras has zero tables for the
// rows it lacks and reads them through the zero-record resource, so their
// syndromes are zero and pass every test (the finish kernel limits "alive" to
// the object's own positions).
template <int X, bool PAD, int BS, int LAUX>
__device__ __forceinline__ void locate_body(const LocMArgs &a, uint32_t obj, uint32_t chunk, uint64_t order,
                                            uint32_t xobj, constant_ptr<uint32_t> tb) {
    // no lane leaves early: the ballots below count every lane of the wave
    const uint32_t v = chunk * BS + threadIdx.x;
    const bool act = v < a.nvec;
    const uint8_t *ob = a.base + (uint64_t)obj * a.obj_stride;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void *)ob, (short)0, (int)a.span, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsn = __builtin_amdgcn_make_buffer_rsrc((void *)ob, (short)0, 0, 0x00020000);
    const uint32_t K = a.K, XM = PAD ? (uint32_t)X : a.XM;
    auto row_off = [&](uint32_t q) -> uint32_t { return ((uint32_t)(order >> (4u * q)) & 15u) * a.pitch; };

    uint32_t s[X][4];
#pragma unroll
    for (int r = 0; r < X; ++r)
#pragma unroll
        for (int d = 0; d < 4; ++d) s[r][d] = 0;

    // survivors: s[r] ^= C[r][c] (x) row c, four rows' loads issued together
    for (uint32_t c0 = 0; c0 < K; c0 += 4) {
        u32x4 x[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            x[j] = u32x4{0u, 0u, 0u, 0u};
            if (act && c0 + j < K) x[j] = __builtin_amdgcn_raw_buffer_load_b128(rs, v * 16u, row_off(c0 + j), LAUX);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (c0 + j < K) {
#pragma unroll
                for (int d = 0; d < 4; ++d) {
                    const GfIdx g = gf_idx(x[j][d]);
#pragma unroll
                    for (int r = 0; r < X; ++r) s[r][d] = gf_mac(s[r][d], tb + ((c0 + j) * XM + r) * kTabWords, g);
                }
            }
        }
    }
    // extras: identity inputs, row K + t enters syndrome t only
    {
        u32x4 x[X];
#pragma unroll
        for (int t = 0; t < X; ++t) {
            x[t] = u32x4{0u, 0u, 0u, 0u};
            if (act)
                x[t] = __builtin_amdgcn_raw_buffer_load_b128(!PAD || (uint32_t)t < xobj ? rs : rsn, v * 16u,
                                                             row_off(K + t), LAUX);
        }
#pragma unroll
        for (int t = 0; t < X; ++t)
#pragma unroll
            for (int d = 0; d < 4; ++d) s[t][d] ^= x[t][d];
    }
    // bytes past shard_len (row padding) take no part
    const uint32_t valid = (v == a.nvec - 1) ? a.tail : 16u;
    uint32_t any = 0;
#pragma unroll
    for (int r = 0; r < X; ++r)
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            s[r][d] &= tail_mask(d, valid);
            any |= s[r][d];
        }
    if (__builtin_amdgcn_ballot_w64(any != 0) == 0) return;  // wave-uniform: clean vectors end here

    // candidate tests, as gf_locate
    uint32_t m = 0;
    if (any != 0) {
        m = kLocSeen;
        GfIdx g[X][4];
#pragma unroll
        for (int r = 0; r < X; ++r)
#pragma unroll
            for (int d = 0; d < 4; ++d) g[r][d] = gf_idx(s[r][d]);
        for (uint32_t q = 0; q < K; ++q) {
            uint32_t diff = 0;
#pragma unroll
            for (int ra = 0; ra < X; ++ra)
#pragma unroll
                for (int rb = ra + 1; rb < X; ++rb)
#pragma unroll
                    for (int d = 0; d < 4; ++d)
                        diff |= gf_mulc(tb + (q * XM + rb) * kTabWords, g[ra][d]) ^
                                gf_mulc(tb + (q * XM + ra) * kTabWords, g[rb][d]);
            if (diff) m |= 1u << q;
        }
        uint32_t nzr[X];
#pragma unroll
        for (int r = 0; r < X; ++r) nzr[r] = s[r][0] | s[r][1] | s[r][2] | s[r][3];
#pragma unroll
        for (int t = 0; t < X; ++t) {
            uint32_t other = 0;
#pragma unroll
            for (int r = 0; r < X; ++r)
                if (r != t) other |= nzr[r];
            if (other) m |= 1u << (K + t);
        }
    }
    uint32_t wm = 0;
#pragma unroll
    for (int i = 0; i <= 16; ++i)
        if (__builtin_amdgcn_ballot_w64(((m >> i) & 1u) != 0) != 0) wm |= 1u << i;
    if ((threadIdx.x & 63u) == 0) atomicOr(&a.acc[obj], wm);
}

// XM: the code's largest X.  PAD = false branches (wave-uniformly) into the
// body of the object's own X; PAD = true runs the XM body for every object.
template <int XM, bool PAD, int BS, int LAUX>
__global__ __launch_bounds__(BS) void gf_locate_masked(const LocMArgs a) {
    uint32_t obj, chunk;
    if (!wg_item(a.ord, obj, chunk)) return;
    // constant address space: mask, slot and the slot's record are uniform
    // and invariant, fetched with s_load (as gf_apply_masked)
    const uint32_t mask = ((constant_ptr<uint32_t>)a.present)[obj] & a.nmask;
    const int32_t slot = ((constant_ptr<int32_t>)a.pat)[mask];
    if (slot < 0) return;  // not served: no load; the finish kernel writes the code
    const constant_ptr<uint32_t> rw = (constant_ptr<uint32_t>)((constant_ptr<LocRec>)a.recs + (uint32_t)slot);
    const uint32_t X = rw[0];
    const uint64_t order = (uint64_t)rw[2] | ((uint64_t)rw[3] << 32);
    const constant_ptr<uint32_t> tb = (constant_ptr<uint32_t>)a.tabs + (size_t)(uint32_t)slot * (a.K * a.XM * kTabWords);
    if constexpr (PAD) {
        locate_body<XM, true, BS, LAUX>(a, obj, chunk, order, X, tb);
    } else {
        if (XM >= 4 && X == 4) locate_body<(XM >= 4 ? 4 : 2), false, BS, LAUX>(a, obj, chunk, order, X, tb);
        else if (XM >= 3 && X == 3) locate_body<(XM >= 3 ? 3 : 2), false, BS, LAUX>(a, obj, chunk, order, X, tb);
        else locate_body<2, false, BS, LAUX>(a, obj, chunk, order, X, tb);
    }
}

__global__ __launch_bounds__(256) void gf_locate_finish_masked(uint32_t *acc, uint32_t nobj, const uint32_t *present,
                                                               const int32_t *pat, const LocRec *recs, uint32_t nmask,
                                                               uint32_t K, int32_t *loc, uint32_t *masks) {
    const uint32_t o = blockIdx.x * 256u + threadIdx.x;
    if (o >= nobj) return;
    const uint32_t w = acc[o];
    if (w && (const void *)acc != (const void *)loc) acc[o] = 0u;  // (as gf_locate_finish)
    uint32_t mask = present[o] & nmask;  // read before masks[o], which may be the same word, is written
    const int32_t slot = pat[mask];
    int32_t r = slot;  // not served: the table's code (its workgroups OR-ed nothing)
    if (slot >= 0) {
        r = kLocClean;
        if (w) {
            const LocRec &rc = recs[slot];
            const uint32_t alive = ~w & ((1u << (K + rc.X)) - 1u);  // the object's own k + X positions
            r = kLocUnlocatable;
            if (__builtin_popcount(alive) == 1) {
                const uint32_t q = (uint32_t)__builtin_ctz(alive);
                r = (int32_t)((rc.order[q >> 3] >> (4u * (q & 7u))) & 15u);
                mask &= ~(1u << r);
            }
        }
    }
    loc[o] = r;
    if (masks) masks[o] = mask;
}

struct LocLArgs {  // short rows: gf_locate_lanes
    const uint8_t *base;
    uint64_t obj_stride;
    const uint32_t *present;
    const int32_t *pat;
    const LocRec *recs;
    const uint32_t *ctab;  // [256][kCtabStride]
    int32_t *loc;
    uint32_t *masks;       // nullable; may be `present`
    uint32_t nmask, K;
    uint32_t nvec, tail, pitch;
    uint32_t opw, nobj, gspan;  // objects per workgroup, batch size, group span (as gf_apply_lanes)
    Order ord;                  // item = group of opw objects
};

// dword i (uniform) of a vector held in VGPRs, by compares (a runtime index
// would put the vector in private memory)
__device__ __forceinline__ uint32_t pick4(const u32x4 &w, uint32_t i) {
    return i == 0 ? w[0] : i == 1 ? w[1] : i == 2 ? w[2] : w[3];
}

// Short rows: one workgroup locates opw = 256 / nvec whole objects in address
// order, lane -> (object, vector), whatever their patterns.  Each lane walks
// the set bits of its own object's mask (the first K are the survivors, the
// next X the extras: `order` is the set bits in ascending order), takes C's
// bytes from its record and multiplies through the 256-entry coefficient
// table staged in LDS.  The dead-position masks are OR-ed per object in LDS
// (an object's lanes can straddle a wave boundary), and one lane per object
// writes the result: no global scratch, no atomics to HBM, no finish kernel.
template <int XM, int LAUX>
__global__ __launch_bounds__(256) void gf_locate_lanes(const LocLArgs a) {
    __shared__ u32x4 lt[256][2];    // coefficient c: lt[c][0] = table words 0-3, lt[c][1].x = word 4
    __shared__ uint32_t lacc[256];  // per object of the group: dead positions | kLocSeen
    uint32_t grp, chunk;
    if (!wg_item(a.ord, grp, chunk)) return;
    const uint32_t t = threadIdx.x;
    const u32x4 *ct = (const u32x4 *)(a.ctab + t * kCtabStride);
    const u32x4 ct0 = ct[0], ct1 = ct[1];

    const uint32_t j = t / a.nvec, v = t - j * a.nvec, o = grp * a.opw + j;
    const bool live = j < a.opw && o < a.nobj;
    // every lane of an object reads its mask here, before the barriers; the
    // one lane that may overwrite the word (masks == present) does so after them
    const uint32_t mask = live ? a.present[o] & a.nmask : 0u;
    const int32_t slot = live ? a.pat[mask] : kLocTooFew;
    const bool act = slot >= 0;
    const uint32_t K = a.K;
    const uint32_t X = act ? (uint32_t)__builtin_popcount(mask) - K : 0u;
    const u32x4 zero = {0u, 0u, 0u, 0u};
    const u32x4 *rp = (const u32x4 *)(a.recs + (act ? (uint32_t)slot : 0u));
    u32x4 crow[XM];  // C[r][0..15] of this lane's pattern
#pragma unroll
    for (int r = 0; r < XM; ++r) crow[r] = act ? rp[1 + r] : zero;

    lt[t][0] = ct0;
    lt[t][1] = ct1;
    lacc[t] = 0u;
    __syncthreads();

    const uint8_t *gb = a.base + (uint64_t)grp * a.opw * a.obj_stride;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void *)gb, (short)0, (int)a.gspan, 0x00020000);
    const uint32_t lane_off = j * (uint32_t)a.obj_stride + v * 16u;
    const uint32_t none = 0xfffffff0u;  // past every range: the load returns zero and touches no memory

    uint32_t s[XM][4];
#pragma unroll
    for (int r = 0; r < XM; ++r)
#pragma unroll
        for (int d = 0; d < 4; ++d) s[r][d] = 0;
    uint32_t m = mask;
    for (uint32_t c0 = 0; c0 < K; c0 += 4) {
        u32x4 x[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const bool use = act && c0 + i < K;
            const uint32_t row = m ? (uint32_t)__builtin_ctz(m) : 0u;
            if (c0 + i < K) m &= m - 1u;
            x[i] = __builtin_amdgcn_raw_buffer_load_b128(rs, use ? lane_off + row * a.pitch : none, 0u, LAUX);
        }
        uint32_t cw[XM];  // coefficient bytes of inputs c0 .. c0 + 3
#pragma unroll
        for (int r = 0; r < XM; ++r) cw[r] = pick4(crow[r], c0 >> 2);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (c0 + i < K) {
                GfIdx g[4];
#pragma unroll
                for (int d = 0; d < 4; ++d) g[d] = gf_idx(x[i][d]);
#pragma unroll
                for (int r = 0; r < XM; ++r) {
                    if (r < kLocMinX || __builtin_amdgcn_ballot_w64((uint32_t)r < X) != 0) {  // some lane has row r
                        const uint32_t cf = (cw[r] >> (8 * i)) & 0xffu;
                        const u32x4 tw = lt[cf][0];
                        const uint32_t t4 = lt[cf][1][0];
#pragma unroll
                        for (int d = 0; d < 4; ++d) s[r][d] = gf_mac_w(s[r][d], tw, t4, g[d]);
                    }
                }
            }
        }
    }
    {  // extras: the next X set bits
        u32x4 x[XM];
#pragma unroll
        for (int e = 0; e < XM; ++e) {
            const uint32_t row = m ? (uint32_t)__builtin_ctz(m) : 0u;
            m &= m - 1u;
            x[e] = __builtin_amdgcn_raw_buffer_load_b128(rs, (uint32_t)e < X ? lane_off + row * a.pitch : none, 0u, LAUX);
        }
#pragma unroll
        for (int e = 0; e < XM; ++e)
#pragma unroll
            for (int d = 0; d < 4; ++d) s[e][d] ^= x[e][d];
    }
    const uint32_t valid = (v == a.nvec - 1) ? a.tail : 16u;
    uint32_t any = 0;
#pragma unroll
    for (int r = 0; r < XM; ++r)
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            s[r][d] &= tail_mask(d, valid);
            any |= s[r][d];
        }
    // candidate tests as gf_locate; rows a lane lacks have zero coefficients
    // and zero syndromes and pass every test
    if (any != 0) {
        uint32_t dead = kLocSeen;
        for (uint32_t q = 0; q < K; ++q) {
            u32x4 tw[XM];
            uint32_t t4[XM];
#pragma unroll
            for (int r = 0; r < XM; ++r) {
                const uint32_t cf = (pick4(crow[r], q >> 2) >> (8u * (q & 3u))) & 0xffu;
                tw[r] = lt[cf][0];
                t4[r] = lt[cf][1][0];
            }
            uint32_t diff = 0;
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                GfIdx g[XM];
#pragma unroll
                for (int r = 0; r < XM; ++r) g[r] = gf_idx(s[r][d]);
#pragma unroll
                for (int ra = 0; ra < XM; ++ra)
#pragma unroll
                    for (int rb = ra + 1; rb < XM; ++rb)
                        diff |= gf_mac_w(0u, tw[rb], t4[rb], g[ra]) ^ gf_mac_w(0u, tw[ra], t4[ra], g[rb]);
            }
            if (diff) dead |= 1u << q;
        }
        uint32_t nzr[XM];
#pragma unroll
        for (int r = 0; r < XM; ++r) nzr[r] = s[r][0] | s[r][1] | s[r][2] | s[r][3];
#pragma unroll
        for (int e = 0; e < XM; ++e) {
            uint32_t other = 0;
#pragma unroll
            for (int r = 0; r < XM; ++r)
                if (r != e) other |= nzr[r];
            if (other) dead |= 1u << (K + e);
        }
        atomicOr(&lacc[j], dead);  // LDS
    }
    __syncthreads();
    if (!live || v != 0) return;
    // one lane per object writes its result
    int32_t r = slot;  // not served: the table's code
    uint32_t om = mask;
    if (act) {
        const uint32_t w = lacc[j];
        r = kLocClean;
        if (w) {
            const uint32_t alive = ~w & ((1u << (K + X)) - 1u);
            r = kLocUnlocatable;
            if (__builtin_popcount(alive) == 1) {
                uint32_t mm = mask;  // column position q holds the q-th present shard
                for (uint32_t q = (uint32_t)__builtin_ctz(alive); q > 0; --q) mm &= mm - 1u;
                r = (int32_t)__builtin_ctz(mm);
                om &= ~(1u << r);
            }
        }
    }
    a.loc[o] = r;
    if (a.masks) a.masks[o] = om;
}

int env_int(const char *name, int dflt) {
    const char *e = std::getenv(name);
    return e && *e ? std::atoi(e) : dflt;
}
// read once at load: RSGPU_LOCATE_LANES=0 forces the long-row form;
// RSGPU_LOCATE_XPAD=1 runs the long-row kernel's largest-X body for every
// object instead of branching on the object's X (measurement)
const int g_locate_lanes = env_int("RSGPU_LOCATE_LANES", 1);
const int g_locate_xpad = env_int("RSGPU_LOCATE_XPAD", 0);

template <int XM, bool PAD>
hipError_t launch_locate_masked_t(const LocAtlasView &A, const Layout &L, const uint32_t *present, uint32_t *acc,
                                  hipStream_t st) {
    LocMArgs a{};
    a.obj_stride = L.obj_stride;
    a.pat = A.pat;
    a.recs = A.recs;
    a.tabs = A.tabs;
    a.nmask = (1u << A.n) - 1u;
    a.K = (uint32_t)A.k;
    a.XM = (uint32_t)A.xmax;
    a.nvec = (uint32_t)((L.shard_len + 15) / 16);
    a.tail = (uint32_t)(L.shard_len - (size_t)(a.nvec - 1) * 16);
    a.pitch = (uint32_t)L.pitch;
    a.span = (uint32_t)((size_t)(A.n - 1) * L.pitch + (size_t)a.nvec * 16);
    const unsigned gx = (a.nvec + kBlock - 1) / kBlock;
    const int step = max_items(gx);
    for (int o0 = 0; o0 < L.nobj; o0 += step) {
        const int no = std::min(step, L.nobj - o0);
        a.base = L.base + (size_t)o0 * L.obj_stride;
        a.present = present + o0;
        a.acc = acc + o0;
        unsigned grid;
        a.ord = make_order(gx, (uint32_t)no, objs_span(L, no, a.span), grid);
        hipLaunchKernelGGL((gf_locate_masked<XM, PAD, kBlock, kLoadAux>), dim3(grid), dim3(kBlock), 0, st, a);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

template <int XM>
hipError_t launch_locate_lanes_t(const LocAtlasView &A, const Layout &L, const uint32_t *present, int32_t *loc,
                                 uint32_t *masks, hipStream_t st) {
    LocLArgs a{};
    a.obj_stride = L.obj_stride;
    a.pat = A.pat;
    a.recs = A.recs;
    a.ctab = A.ctab;
    a.nmask = (1u << A.n) - 1u;
    a.K = (uint32_t)A.k;
    a.nvec = (uint32_t)((L.shard_len + 15) / 16);
    a.tail = (uint32_t)(L.shard_len - (size_t)(a.nvec - 1) * 16);
    a.pitch = (uint32_t)L.pitch;
    const uint32_t span = (uint32_t)((size_t)(A.n - 1) * L.pitch + (size_t)a.nvec * 16);
    // all lanes of a group address its objects from the first one in one
    // 32-bit range (as launch_masked_t)
    uint32_t opw = kBlock / a.nvec;
    while (opw > 1 && (uint64_t)(opw - 1) * L.obj_stride + span >= 0x7fffffffull) opw /= 2;
    a.opw = opw;
    a.gspan = (uint32_t)((uint64_t)(opw - 1) * L.obj_stride + span);
    const size_t groups = ((size_t)L.nobj + opw - 1) / opw;
    for (size_t g0 = 0; g0 < groups; g0 += (size_t)max_items(1)) {
        const size_t ng = std::min((size_t)max_items(1), groups - g0);
        const size_t o0 = g0 * opw;
        a.base = L.base + o0 * L.obj_stride;
        a.present = present + o0;
        a.loc = loc + o0;
        a.masks = masks ? masks + o0 : nullptr;
        a.nobj = (uint32_t)std::min<size_t>(ng * opw, (size_t)L.nobj - o0);
        unsigned grid;
        a.ord = make_order(1, (uint32_t)ng, (size_t)a.nobj * L.obj_stride, grid);
        hipLaunchKernelGGL((gf_locate_lanes<XM, kLoadAux>), dim3(grid), dim3(kBlock), 0, st, a);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace

bool locate_lanes_form(const Layout &L) {
    const size_t nvec = (L.shard_len + 15) / 16;
    return g_locate_lanes != 0 && L.nobj > 1 && nvec * 2 <= (size_t)kBlock;
}

hipError_t launch_locate_masks(const LocAtlasView &A, const Layout &L, const uint32_t *present, uint32_t *acc,
                               int32_t *loc, uint32_t *masks, hipStream_t st, bool clear) {
    if (L.nobj <= 0) return hipSuccess;
    if (A.n < 1 || A.n > kLocMaxN || A.k < 1 || A.k >= A.n || A.xmax < kLocMinX || A.xmax > kLocMaxX ||
        (L.pitch % 16) != 0 || L.shard_len == 0)
        return hipErrorInvalidValue;
    if (locate_lanes_form(L))
        return A.xmax == 2 ? launch_locate_lanes_t<2>(A, L, present, loc, masks, st)
             : A.xmax == 3 ? launch_locate_lanes_t<3>(A, L, present, loc, masks, st)
                           : launch_locate_lanes_t<4>(A, L, present, loc, masks, st);
    if (clear) {
        hipError_t e = launch_zero_u32(acc, (size_t)L.nobj, st);
        if (e != hipSuccess) return e;
    }
    const bool pad = g_locate_xpad != 0;
    hipError_t e = A.xmax == 2 ? launch_locate_masked_t<2, false>(A, L, present, acc, st)
                 : A.xmax == 3 ? (pad ? launch_locate_masked_t<3, true>(A, L, present, acc, st)
                                      : launch_locate_masked_t<3, false>(A, L, present, acc, st))
                               : (pad ? launch_locate_masked_t<4, true>(A, L, present, acc, st)
                                      : launch_locate_masked_t<4, false>(A, L, present, acc, st));
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(gf_locate_finish_masked, dim3(((unsigned)L.nobj + 255u) / 256u), dim3(256), 0, st, acc,
                       (uint32_t)L.nobj, present, A.pat, A.recs, (1u << A.n) - 1u, (uint32_t)A.k, loc, masks);
    return hipGetLastError();
}

hipError_t launch_zero_u32(uint32_t *p, size_t n, hipStream_t st) {
    for (size_t i = 0; i < n; i += (size_t)1 << 30) {
        const uint32_t m = (uint32_t)std::min(n - i, (size_t)1 << 30);
        hipLaunchKernelGGL(gf_locate_clear, dim3((m + 255u) / 256u), dim3(256), 0, st, p + i, m);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_locate(const LocPlan &P, const Layout &L, uint32_t *acc, int32_t *loc, uint32_t *masks,
                         hipStream_t st, bool clear) {
    if (L.nobj <= 0) return hipSuccess;
    if (P.X < kLocMinX || P.X > kLocMaxX || P.K < 1 || P.K + P.X > kLocMaxN || P.nrows > kLocMaxN ||
        (L.pitch % 16) != 0)
        return hipErrorInvalidValue;
    uint64_t order = 0;
    for (int q = 0; q < P.K + P.X; ++q) order |= (uint64_t)(P.order[q] & 15u) << (4 * q);
    const dim3 per_obj(((unsigned)L.nobj + 255u) / 256u);
    if (clear) {
        hipError_t e = launch_zero_u32(acc, (size_t)L.nobj, st);
        if (e != hipSuccess) return e;
    }
    hipError_t e = P.X == 2 ? launch_locate_t<2>(P, L, acc, order, st)
                 : P.X == 3 ? launch_locate_t<3>(P, L, acc, order, st)
                            : launch_locate_t<4>(P, L, acc, order, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(gf_locate_finish, per_obj, dim3(256), 0, st, acc,
                       (uint32_t)L.nobj, (uint32_t)(P.K + P.X), order, P.present, loc, masks);
    return hipGetLastError();
}

}  // namespace rsgpu
