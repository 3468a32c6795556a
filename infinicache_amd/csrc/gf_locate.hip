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
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "gf_device.h"
#include "gf_launch.h"
#include "gf_locate.h"

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

}  // namespace

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
