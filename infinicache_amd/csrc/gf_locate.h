// gf_locate.h — the corrupted-shard locator (gf_locate.hip): a second use of
// the fused decode's check rows.
//
// For one erasure pattern, Q = the present shards in index order, S = the
// first k of them (the survivors), E = the remaining X = |Q| - k extras,
// C = G[E] x inv(G[S]) (X x k) and H = [C | I_X] over the columns S then E.
// s(c) = H x y(c) are the X syndromes of byte column c: exactly the check
// rows of build_reconstruct(..., check = true).  A single corrupted shard at
// column position q makes every s(c) a multiple of column q of H; with X >= 2
// and an MDS code no two columns are parallel, so the position is unique.
#pragma once
#include <cstdint>

#include <hip/hip_runtime_api.h>

#include "gf_apply.h"

namespace rsgpu {

constexpr int kLocMaxN = 16;  // shards of a code the locator serves
constexpr int kLocMinX = 2;   // extras: fewer cannot tell which shard is bad
constexpr int kLocMaxX = 4;
// per-object scratch word the locate kernel ORs into: bit q < k + X = column
// position q is dead (some byte column's syndromes are not parallel to it),
// kLocSeen = some syndrome byte is non-zero
constexpr uint32_t kLocSeen = 1u << 16;
constexpr int32_t kLocClean = -1, kLocUnlocatable = -2;  // RSGPU_LOC_*

// One erasure pattern's locator, host side (rsgpu.cpp build_locate)
struct LocPlan {
    int K = 0, X = 0;             // survivors, extras
    int nrows = 0;                // shards of the code (rows of an object)
    uint8_t order[kLocMaxN] = {}; // column position -> shard index (S then E)
    uint32_t present = 0;         // bit i: shard i present
    // [c][r][kCoefWords]: the table of C[r][c], as Pass::tab (input-major)
    uint32_t tab[(kLocMaxN - kLocMinX) * kLocMaxX * kCoefWords] = {};
};

// Locates on `stream`: acc (L.nobj u32) collects the dead-position masks: all
// zero and left zero (the status ring), or any words, loc itself included,
// with clear = true (a kernel zeroes them first).  The finish kernel writes
// loc[o] (kLocClean, kLocUnlocatable or the shard index) and, when masks !=
// nullptr, masks[o] = the present mask with the located shard cleared.
hipError_t launch_locate(const LocPlan &P, const Layout &L, uint32_t *acc, int32_t *loc, uint32_t *masks,
                         hipStream_t stream, bool clear = false);


// Zeroes n words with a kernel on `stream`.  For stream captures: a replayed
// graph's memset nodes were seen not to have zeroed small counters before the
// kernels that follow them read them (tests/test_gpu_locate.py's graph test
// finds stale words), kernel-to-kernel order holds.
hipError_t launch_zero_u32(uint32_t *p, size_t n, hipStream_t stream);

}  // namespace rsgpu
