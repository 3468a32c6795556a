"""Per-object corrupted-shard location (rsgpu_locate_pattern,
rsgpu_locate_dev_masks, rsgpu_repair_dev_masks), the parts that need no GPU:
the header and exports, rsgpu_locate_pattern over every mask of a code against
a numpy classification built from the oracle's matrices, and the call-level
error table of include/rsgpu.h, returned before any device is touched."""
import ctypes
import functools
import re

import numpy as np
import pytest

import infinicache_amd as ia
from infinicache_amd import _lib
from oracle import rs_numpy as rn

TOO_FEW, TOO_MANY, SINGULAR = -3, -4, -5


@functools.lru_cache(maxsize=None)
def classify(k, p, kind):
    """What the locator makes of every mask of the code, from the oracle:
    X (2..4) when served, else TOO_FEW, TOO_MANY, SINGULAR in that order
    (singular: G[Q[:k]] has no inverse, Q the present shards in index order)."""
    n = k + p
    G = rn.build_matrix(k, p, kind)
    out = np.empty(1 << n, dtype=np.int32)
    for mask in range(1 << n):
        Q = [i for i in range(n) if mask >> i & 1]
        if len(Q) < k + 2:
            out[mask] = TOO_FEW
        elif len(Q) - k > 4:
            out[mask] = TOO_MANY
        else:
            try:
                rn.invert(G[Q[:k]])
                out[mask] = len(Q) - k
            except rn.Singular:
                out[mask] = SINGULAR
    out.setflags(write=False)
    return out


def _header():
    return open(_lib.HEADER).read()


def test_header_and_exports():
    src = _header()
    for name, value in (("RSGPU_LOC_TOO_FEW", TOO_FEW), ("RSGPU_LOC_TOO_MANY", TOO_MANY),
                        ("RSGPU_LOC_SINGULAR", SINGULAR)):
        m = re.search(r"#define %s\s+\((-?\d+)\)" % name, src)
        assert m and int(m[1]) == value, name
    L = _lib.load()
    for fn in ("rsgpu_locate_pattern", "rsgpu_locate_dev_masks", "rsgpu_repair_dev_masks"):
        assert re.search(r"\bint %s\(rsgpu_ctx \*ctx" % fn, src), fn
        assert fn in _lib.EXPORTS
        assert getattr(L, fn).argtypes is not None
    assert (ia.LOC_TOO_FEW, ia.LOC_TOO_MANY, ia.LOC_SINGULAR) == (TOO_FEW, TOO_MANY, SINGULAR)
    for name in ("LOC_TOO_FEW", "LOC_TOO_MANY", "LOC_SINGULAR"):
        assert name in ia.__all__
    enc = ia.New(10, 2)
    for meth in ("locate_pattern", "locate_dev_masks", "repair_dev_masks"):
        assert callable(getattr(enc, meth))


# (k, p, kind, served by X = 2, 3, 4, too many, singular masks the oracle must find)
PATTERN_CODES = [
    (10, 2, "vandermonde", (1, 0, 0), 0, ()),
    (10, 4, "vandermonde", (91, 14, 1), 0, ()),
    (6, 3, "vandermonde", (9, 1, 0), 0, ()),
    (4, 6, "vandermonde", (210, 120, 45), 11, ()),
    (10, 4, "cauchy", (91, 14, 1), 0, ()),
    (3, 6, "par1", None, None, (0x1d8,)),
    (5, 6, "par1", None, None, (0x766, 0x778)),
]


@pytest.mark.parametrize("k,p,kind,served,too_many,singular", PATTERN_CODES)
def test_locate_pattern_every_mask(k, p, kind, served, too_many, singular):
    n = k + p
    want = classify(k, p, kind)
    # the oracle's own counts first
    if served is not None:
        assert tuple(int((want == x).sum()) for x in (2, 3, 4)) == served
        assert int((want == TOO_MANY).sum()) == too_many
        assert int((want == SINGULAR).sum()) == 0
        assert int((want == TOO_FEW).sum()) == (1 << n) - sum(served) - too_many
    for m in singular:
        assert want[m] == SINGULAR, hex(m)
    if (k, p) == (10, 2):
        assert want[0xFFF] == 2
    if (k, p, kind) == (10, 4, "vandermonde"):
        assert int((want == TOO_FEW).sum()) == 16278
    enc = ia.New(k, p, matrix=kind)
    L = _lib.load()
    got = np.array([L.rsgpu_locate_pattern(enc._ctx, m) for m in range(1 << n)], dtype=np.int32)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, [(hex(int(m)), int(got[m]), int(want[m])) for m in bad[:8]]
    # the Python mirror, and bits >= n ignored
    for m in (0, (1 << n) - 1, *singular, *np.flatnonzero(want >= 2)[:3].tolist()):
        assert enc.locate_pattern(m) == want[m]
        assert enc.locate_pattern((m | 0xA5 << n) & 0xFFFFFFFF) == want[m]
        assert L.rsgpu_locate_pattern(enc._ctx, (m | 0xFFFFFFFF << n) & 0xFFFFFFFF) == want[m]
    # served masks: X is rsgpu_check_matrix's x_out
    for m in np.flatnonzero(want >= 2):
        H, order = enc.check_matrix([int(m) >> i & 1 for i in range(n)])
        assert H.shape[0] == want[m] and len(order) == k + want[m], hex(int(m))
    # unserved masks: rsgpu_check_matrix refuses them with the matching error
    for code, err in ((TOO_FEW, ia.ErrTooFewShards), (TOO_MANY, ia.ErrNotImplemented), (SINGULAR, ia.ErrSingular)):
        for m in np.flatnonzero(want == code)[-2:]:
            with pytest.raises(err):
                enc.check_matrix([int(m) >> i & 1 for i in range(n)])


def _codes():
    return dict((m[0], int(m[1])) for m in re.findall(r"#define (RSGPU_ERR_\w+) (-?\d+)", _header()))


def test_locate_pattern_errors():
    L = _lib.load()
    E = _codes()
    assert L.rsgpu_locate_pattern(None, 0xFFF) == E["RSGPU_ERR_INVALID_ARG"]
    enc17 = ia.New(14, 3)
    for m in (0, 0x1FFFF, 0xFFFF):
        assert L.rsgpu_locate_pattern(enc17._ctx, m) == E["RSGPU_ERR_NOT_IMPLEMENTED"]
    with pytest.raises(ia.ErrNotImplemented):
        enc17.locate_pattern(0x1FFFF)


def test_error_precedence_without_device():
    """Each row of the header's call-level table, in its order, for both
    calls; none reaches a device (the pointers are never read)."""
    L = _lib.load()
    E = _codes()
    base, out = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 24)
    INV, NOTIMPL, NODATA = E["RSGPU_ERR_INVALID_ARG"], E["RSGPU_ERR_NOT_IMPLEMENTED"], E["RSGPU_ERR_SHARD_NO_DATA"]

    def calls(enc, ctx="own", base=base, present=out, S=64, pitch=64, stride=None, nobj=2, loc=out, masks=out,
              status=out):
        n = enc.Shards
        stride = n * pitch if stride is None else stride
        ctx = enc._ctx if ctx == "own" else ctx
        return {
            "locate": L.rsgpu_locate_dev_masks(ctx, base, present, S, pitch, stride, nobj, loc, masks, None),
            "repair": L.rsgpu_repair_dev_masks(ctx, base, present, S, pitch, stride, nobj, loc, masks, status, None),
        }

    def all_are(res, code, names=("locate", "repair")):
        for name in names:
            assert res[name] == code, (name, res[name], code)

    enc, enc17 = ia.New(10, 4), ia.New(14, 3)
    # 1. NULL ctx or d_present: before everything else
    all_are(calls(enc, ctx=None), INV)
    all_are(calls(enc17, present=None, S=0, loc=None), INV)
    # 2. more than 16 shards: before the layout and the result pointers
    all_are(calls(enc17), NOTIMPL)
    all_are(calls(enc17, S=0, pitch=100, loc=None, masks=None, status=None), NOTIMPL)
    # 3. layout: no data, then misaligned or oversized; before the result pointers
    all_are(calls(enc, S=0, loc=None, masks=None, status=None), NODATA)
    all_are(calls(enc, S=0, pitch=100), NODATA)
    all_are(calls(enc, S=100, pitch=100), INV)                                   # pitch % 16
    all_are(calls(enc, S=100, pitch=112, stride=14 * 112 + 8), INV)              # stride % 16
    all_are(calls(enc, base=ctypes.c_void_p((1 << 20) + 8)), INV)                # base % 16
    all_are(calls(enc, S=100, pitch=96), INV)                                    # pitch < S
    all_are(calls(enc, base=ctypes.c_void_p(0)), INV)
    all_are(calls(enc, pitch=400 << 20), INV)                                    # 14 rows >= 4 GiB
    all_are(calls(enc, nobj=-1), INV)
    # 4. result pointers (d_masks is optional for locate, required for repair)
    all_are(calls(enc, loc=None), INV)
    all_are(calls(enc, masks=None), INV, ("repair",))
    all_are(calls(enc, status=None), INV, ("repair",))
    # 5. a valid call gets as far as the device, and no further without one
    if not ia.device_ok(0):
        all_are(calls(enc), E["RSGPU_ERR_NO_DEVICE"])
        all_are(calls(enc, masks=None), E["RSGPU_ERR_NO_DEVICE"], ("locate",))
        all_are(calls(ia.New(10, 1)), E["RSGPU_ERR_NO_DEVICE"])  # no pattern served: still no call-level error
        with pytest.raises(ia.NoDevice):
            enc.locate_dev_masks(1 << 20, 1 << 24, 64, 64, 14 * 64, 2, 1 << 24)
        with pytest.raises(ia.NoDevice):
            enc.repair_dev_masks(1 << 20, 1 << 24, 64, 64, 14 * 64, 2, 1 << 24, 1 << 24, 1 << 24)
