"""Every specialised (K, R) kernel in every launch form, bit-exact against
the oracles (oracle/rs_numpy.py for the matrices and inversions, liboracle
for the byte coding), on the same input bytes.  No tolerances.

Every device operation with K <= 16 inputs runs a kernel compiled for its own
(K, R): pick_fixed / pick_stage / pick_var (csrc/gf_kernels.hip) and
pick_masked (csrc/gf_masked.hip), K = 1..16 by R = 1..4 each.  The sweeps
below reach each of them, per operation:

  encode_dev       K = k,     R = p,     ki = 0, nw = R
  verify_dev       K = k + p, R = p,     ki = p, nw = 0
  reconstruct_dev  K = k,     R = e,     ki = 0, nw = R   (e rows lost)
  decode_dev       K = k + x, R = e + x, ki = x, 0 < nw < R  (x = p - e extras)

The shapes (S bytes per shard, 16-B vectors, nvec = ceil(S / 16)) are the
smallest that select each launch form.  They are derived from kBlock = 256,
kUnroll = 1, kMultiChunks = 1, kMaxK = 16, kMaxR = 4 (csrc/gf_launch.h) and
kStagedMaxVec = 8 (csrc/gf_device.h); test_form_constants guards those.

  S     pitch nobj  form, and the condition that selects it
  8197  8208  3     chunks, ragged: nvec = 513, so `a.nvec * 2 <= kBlock` in
                    launch_fixed fails and the kFormChunks launch runs with
                    gx = 3 workgroups per row and a 5-byte tail; the same
                    condition in launch_tri (`(shard_len + 15) / 16 * 2 <=
                    kBlock` returns false) admits gf_apply_tri for its six
                    tri_shape()s, and in launch_fixed3 / stage_class /
                    launch_masked_t it selects their chunk layouts
  147   160   1     chunks, one short row: `L.nobj > 1` fails in launch_fixed
                    (and launch_fixed3), so the kFormChunks launch runs with
                    nvec = 10
  147   160   57    small, not staged: nobj > 1 and nvec * 2 <= kBlock in
                    launch_fixed give opw = kBlock / nvec = 25 (two full
                    groups and one of 7); use_staged refuses nvec = 10 >
                    kStagedMaxVec, so kFormSmall runs; the same condition in
                    launch_fixed3, stage_class and launch_masked_t selects
                    their packed (opw > 1) layouts
  103   104   77    small, packed rows: nvec = 7 <= kStagedMaxVec, but
                    tail_part(pitch, nvec) = 8 makes Pass::packed != 0 and
                    use_staged refuses; 16 * nvec > pitch also makes
                    overhangs() true, so launch_plan codes the batch's last
                    object in launch_last_object's scratch copy
  103   112   77    staged: nvec = 7, whole vectors (packed == 0, sub_stride
                    == 0), use_staged accepts: gf_apply_staged, opw = 36
  128   128   33    staged, edge: nvec = 8 == kStagedMaxVec, opw = 32 (one
                    full group and one object)
  1     16    5     one byte: nvec = 1, tail = 1 (staged form, opw = 256)

Check-only passes with R >= 3 and K - ki >= 6 (use_triples) go to
launch_fixed3 (Pass3 tables from fill_triples, K - ki mod 3 single-input
leftovers) in its small and chunks layouts; codes with more than kMaxR
parity rows run a second pass with r0 = 4 (launch_plan_core), and fill_pass
applies ki to a plan's last pass only.

Every object lies between two 256-byte guard zones of 0xC3.  Before each
call the pad bytes [S, pitch) of every row and the rows that are lost or
about to be written hold seeded random garbage.  After each call the guards
and every row the operation does not write are unchanged over their full
pitch, and every written row equals the reference on [0, S).

The other families run over the same (k, p) grid: *_dev_multi (the calls as
the API routes them, and once more from a base that is not 16-B aligned,
which recon_dev_multi sends to the host-planned launch_plans_multi ->
stage_class -> gf_apply_multi for every code), *_dev_objs (launch_plan_objs
-> gf_apply_var; a pitch below roundup16(S) is outside their contract, and
the refusal is asserted), *_dev_masks (launch_masked_t: gf_apply_lanes for
nvec * 2 <= kBlock, gf_apply_masked beyond; objects with more than p rows
lost get the documented status 2 and stay untouched) and the host calls on
pinned Split images (run_host_once redirects the pass's loads and stores:
kFormRedirect).

RSGPU_TRI, RSGPU_STAGED and RSGPU_TRIPLES are read once at load: the kernels
behind them run in one fresh child process per setting."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import infinicache_amd as ia
import oracle
from oracle import rs_numpy as rn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu_test = pytest.mark.gpu

GUARD = 256
GUARD_BYTE = 0xC3

CHUNKS = (8197, 8208, 3)
ONE_ROW = (147, 160, 1)
SMALL = (147, 160, 57)
PACKED = (103, 104, 77)
STAGED = (103, 112, 77)
STAGED_EDGE = (128, 128, 33)
ONE_BYTE = (1, 16, 5)
SHAPES = (CHUNKS, ONE_ROW, SMALL, PACKED, STAGED, STAGED_EDGE, ONE_BYTE)
MULTI_SHAPES = (SMALL, (8197, 8208, 6))
MASK_SHAPES = (SMALL, (4197, 4208, 9))
VAR_OBJS = ((1, 16), (103, 112), (147, 160), (4099, 4112), (8197, 8224))  # (S, pitch), each its own
VAR_PACKED = (103, 104)  # pitch == S rounded up to 4: below roundup16(S), which the *_dev_objs calls refuse
HOST_S = 4099

KS = tuple(range(1, 17))
PS = (1, 2, 3, 4)
OPS = ("encode", "verify", "reconstruct", "decode")
TWO_PASS_KS = (1, 5, 6, 11, 16)
TWO_PASS_PS = (5, 6, 7, 8)
TRIPLE_KS = (6, 7, 8, 10, 13)

CONSTANTS = {"kBlock": 256, "kUnroll": 1, "kMultiChunks": 1, "kMaxK": 16, "kMaxR": 4, "kStagedMaxVec": 8}


# ------------------------------------------------------------ the constants

def test_form_constants():
    """The shapes above select their launch forms only for these values."""
    text = ""
    for name in ("gf_launch.h", "gf_device.h"):
        with open(os.path.join(ROOT, "infinicache_amd", "csrc", name)) as f:
            text += f.read()
    for name, want in CONSTANTS.items():
        found = re.findall(r"constexpr\s+\w+\s+%s\s*=\s*(\d+)\s*;" % name, text)
        assert len(found) == 1, "%s: expected one definition in gf_launch.h / gf_device.h, found %r" % (name, found)
        assert int(found[0]) == want, (
            "%s is %s, not %d: the form table in tests/test_gpu_forms.py (which shape selects which launch "
            "form) must be re-derived from launch_fixed, use_staged, use_triples, launch_tri, stage_class and "
            "launch_masked_t" % (name, found[0], want))


# ------------------------------------------------------------- loss patterns

def _pattern_mixed(k, p, e):
    """e lost rows, data and parity mixed, the survivors non-contiguous:
    odd data rows first (1, 3, ...), parity rows from the last one down in
    steps of two.  e = 1 loses data row 1 (parity row n - 1 when k = 1)."""
    n = k + p
    if e == 1:
        return (1,) if k > 1 else (n - 1,)
    nd = min(k, (e + 1) // 2)
    data = [i for i in list(range(1, k, 2)) + list(range(0, k, 2))][:nd]
    par = list(range(n - 1, k - 1, -2)) + list(range(n - 2, k - 1, -2))
    return tuple(sorted(data + par[:e - nd]))


def _pattern_data(k, p, e):
    """e lost rows, data rows only, from the last one down (when e > k: every
    data row and the first e - k parity rows)."""
    lost = list(range(k - 1, -1, -1))[:e]
    lost += list(range(k, k + e - len(lost)))
    return tuple(sorted(lost))


def _patterns(k, p, e):
    a, b = _pattern_mixed(k, p, e), _pattern_data(k, p, e)
    return (a,) if a == b else (a, b)


def _multi_patterns(k, p):
    """At least four patterns where the code has that many: nothing lost, p
    rows lost, then the others the uniform sweep uses."""
    n = k + p
    out = [(), _pattern_mixed(k, p, p), _pattern_data(k, p, 1), _pattern_mixed(k, p, 1), _pattern_data(k, p, p)]
    out += [_pattern_mixed(k, p, e) for e in range(2, p)] + [(i,) for i in range(n)]
    seen = []
    for pat in out:
        if pat not in seen:
            seen.append(pat)
    return seen[:6]


def _mask_present(k, p, S, nobj):
    """Seeded present flags of the masks sweep: each object loses 0..p random
    rows; objects 3, 14, 25, ... lose p + 1 (too few shards)."""
    n = k + p
    rng = np.random.default_rng([k, p, S, nobj, 77])
    present = np.ones((nobj, n), dtype=np.uint8)
    for o in range(nobj):
        nl = p + 1 if o % 11 == 3 else int(rng.integers(0, p + 1))
        present[o, rng.choice(n, nl, replace=False)] = 0
    return present


# ---------------------------------------------------------------- references

@functools.lru_cache(maxsize=None)
def _matrix(k, p):
    return rn.build_matrix(k, p)


@functools.lru_cache(maxsize=None)
def _inverse(k, p, valid):
    return rn.invert(_matrix(k, p)[list(valid)])  # raises rn.Singular; never for these MDS codes


class Uniform:
    """nobj objects of n rows at one pitch, each between two guard zones."""

    def __init__(self, n, S, pitch, nobj):
        self.n, self.S, self.pitch, self.nobj = n, S, pitch, nobj
        self.body = n * pitch
        self.stride = self.body + 2 * GUARD
        self.size = nobj * self.stride
        self.objs = [(o * self.stride + GUARD, S, pitch) for o in range(nobj)]

    def host(self, rng):
        H = rng.integers(0, 256, (self.nobj, self.stride), dtype=np.uint8)
        H[:, :GUARD] = GUARD_BYTE
        H[:, GUARD + self.body:] = GUARD_BYTE
        return H.reshape(-1)

    def rows(self, A):
        """(nobj, n, pitch) view of the rows of A"""
        return np.ndarray((self.nobj, self.n, self.pitch), np.uint8, buffer=A, offset=GUARD,
                          strides=(self.stride, self.pitch, 1))

    def guards_ok(self, G):
        g = G.reshape(self.nobj, self.stride)
        return bool((g[:, :GUARD] == GUARD_BYTE).all() and (g[:, GUARD + self.body:] == GUARD_BYTE).all())


class Var:
    """objects of their own size and pitch, each between two guard zones"""

    def __init__(self, n, shapes):
        self.n = n
        self.nobj = len(shapes)
        self.objs, off = [], 0
        for S, pitch in shapes:
            self.objs.append((off + GUARD, S, pitch))
            off += n * pitch + 2 * GUARD
        self.size = off
        self.inside = np.zeros(off, dtype=bool)
        for o, S, pitch in self.objs:
            self.inside[o:o + n * pitch] = True

    def host(self, rng):
        H = rng.integers(0, 256, self.size, dtype=np.uint8)
        H[~self.inside] = GUARD_BYTE
        return H

    def rows(self, A):
        return [A[o:o + self.n * pitch].reshape(self.n, pitch) for o, S, pitch in self.objs]

    def guards_ok(self, G):
        return bool((G[~self.inside] == GUARD_BYTE).all())


def _code(lay, A, coef, in_rows, out_rows, sel=None):
    """rows out_rows <- coef x rows in_rows (liboracle), in place in A, for
    the objects sel (default: all)"""
    if not len(out_rows):
        return
    if sel is None and isinstance(lay, Uniform):
        oracle.code_batch(coef, list(in_rows), list(out_rows), A[GUARD:], lay.stride, lay.pitch, lay.S, lay.nobj)
        return
    for o in (range(lay.nobj) if sel is None else sel):
        off, S, pitch = lay.objs[o]
        oracle.code_batch(coef, list(in_rows), list(out_rows), A[off:], 0, pitch, S, 1)


def _ref_encode(lay, k, p, A, sel=None):
    _code(lay, A, _matrix(k, p)[k:], range(k), range(k, k + p), sel)
    return list(range(k, k + p))


def _ref_reconstruct(lay, k, p, A, present, data_only=False, sel=None):
    """upstream reconstruct(): survivors = the first k present rows; missing
    data rows from the inverse, then missing parity rows from the data rows.
    Returns the rows written."""
    n = k + p
    pres = [i for i in range(n) if present[i]]
    assert len(pres) >= k
    if len(pres) == n:
        return []
    valid = tuple(pres[:k])
    miss_data = [i for i in range(k) if not present[i]]
    miss_par = [] if data_only else [i for i in range(k, n) if not present[i]]
    if miss_data:
        _code(lay, A, _inverse(k, p, valid)[miss_data], valid, miss_data, sel)
    if miss_par:
        _code(lay, A, _matrix(k, p)[miss_par], range(k), miss_par, sel)
    return miss_data + miss_par


def _ref_flags(lay, k, p, A):
    """upstream Verify per object: 1 where a parity row differs from the
    data rows' coding"""
    m, n = _matrix(k, p), k + p
    if isinstance(lay, Uniform):
        ok = oracle.verify_batch(m[k:], list(range(k)), list(range(k, n)), A[GUARD:], lay.stride, lay.pitch, lay.S,
                                 lay.nobj)
        return 1 - ok.astype(np.int32)
    out = np.zeros(lay.nobj, dtype=np.int32)
    for o, (off, S, pitch) in enumerate(lay.objs):
        out[o] = 1 - int(oracle.verify_batch(m[k:], list(range(k)), list(range(k, n)), A[off:], 0, pitch, S, 1)[0])
    return out


def _garbage(lay, A, rng, rows, sel=None):
    """seeded random bytes over the full pitch of `rows`"""
    R = lay.rows(A)
    for o in (range(lay.nobj) if sel is None else sel):
        for r in rows:
            R[o][r, :] = rng.integers(0, 256, R[o].shape[1], dtype=np.uint8)


def _flip(lay, A, o, row, j):
    """one bit of object o's row: at byte 0, S - 1 or the first byte of the
    last vector (j picks)"""
    S = lay.objs[o][1]
    pos = (0, S - 1, 16 * ((S + 15) // 16 - 1))[j % 3]
    lay.rows(A)[o][row, pos] ^= 1 << (j % 8)


def _check(lay, G, X, W, written, tag):
    """G (the device's result on X) against the reference W: guards and
    unwritten rows untouched over their full pitch, written rows equal on
    [0, S).  written: row list for every object, or (nobj, n) flags."""
    assert lay.guards_ok(G), (tag, "guard zone written")
    wr = np.zeros((lay.nobj, lay.n), dtype=bool)
    if isinstance(written, np.ndarray):
        wr[:] = written
    else:
        wr[:, list(written)] = True
    g, x, w = lay.rows(G), lay.rows(X), lay.rows(W)
    if isinstance(lay, Uniform):
        if np.array_equal(g[~wr], x[~wr]) and np.array_equal(g[wr][:, :lay.S], w[wr][:, :lay.S]):
            return
    for o in range(lay.nobj):
        S = lay.objs[o][1]
        for r in range(lay.n):
            if wr[o, r]:
                assert np.array_equal(g[o][r, :S], w[o][r, :S]), (tag, "object", o, "written row", r, "differs")
            else:
                assert np.array_equal(g[o][r], x[o][r]), (tag, "object", o, "row", r, "must not change")


# ------------------------------------------------------------------- device

_ENC = {}


def _enc(k, p):
    if (k, p) not in _ENC:
        _ENC[(k, p)] = ia.New(k, p)
    return _ENC[(k, p)]


class Dev:
    """X on the device (shift: bytes the base is moved off 16-B alignment)"""

    def __init__(self, lay, X, shift=0):
        import torch
        self.torch = torch
        self.lay = lay
        self.buf = torch.empty(lay.size + 32, dtype=torch.uint8, device="cuda")
        self.view = self.buf[shift:shift + lay.size]
        self.view.copy_(torch.from_numpy(X))
        self.ptr = self.view.data_ptr()
        self.stream = torch.cuda.current_stream()

    def base(self):  # the first object's first row
        return self.ptr + GUARD

    def objs(self):
        return [(self.ptr + off, S, pitch) for off, S, pitch in self.lay.objs]

    def flags(self, fill=7):
        return self.torch.full((self.lay.nobj,), fill, dtype=self.torch.int32, device="cuda")

    def result(self):
        self.torch.cuda.synchronize()
        return self.view.cpu().numpy()


def _u(lay):  # (shard_len, pitch, obj_stride, nobj) of a uniform layout
    return lay.S, lay.pitch, lay.stride, lay.nobj


CALLS = [0]  # device calls made (the child processes report it)


def _flip_some(lay, X, present, every, first, k):
    """One bit flipped in objects first, first + every, ...: the j-th of them
    in the present row (last + j * k) mod count, so the rows vary over
    parity and data rows.  present: flags for all, or (nobj, n).  Returns the objects."""
    hit = []
    for j, o in enumerate(range(first, lay.nobj, every)):
        pr = present[o] if isinstance(present, np.ndarray) and present.ndim == 2 else present
        rows = [i for i in range(lay.n) if pr[i]]
        if len(rows) < k:
            continue
        _flip(lay, X, o, rows[(len(rows) - 1 + j * k) % len(rows)], j)
        hit.append(o)
    return hit


# --------------------------------------------- section 3: the uniform layout

def sweep_uniform(k, ps=PS, shapes=SHAPES, ops=OPS):
    """encode_dev / verify_dev / reconstruct_dev / decode_dev of RS(k + p)
    for p in ps at every shape, against the references."""
    for p in ps:
        n = k + p
        enc = _enc(k, p)
        for shape in shapes:
            lay = Uniform(n, *shape)
            rng = np.random.default_rng([k, p, *shape])
            C = lay.host(rng)  # random rows and pads, then the reference's parity on [0, S)
            _ref_encode(lay, k, p, C)
            tag = (k, p, shape)
            if "encode" in ops:
                X = C.copy()
                _garbage(lay, X, rng, range(k, n))
                d = Dev(lay, X)
                enc.encode_dev(d.base(), *_u(lay), d.stream)
                CALLS[0] += 1
                _check(lay, d.result(), X, C, range(k, n), tag + ("encode",))
            if "verify" in ops and n <= 16:
                d = Dev(lay, C)
                bad = d.flags()
                enc.verify_dev(d.base(), *_u(lay), bad, d.stream)
                CALLS[0] += 1
                G = d.result()
                assert bad.cpu().tolist() == [0] * lay.nobj, tag + ("verify clean",)
                _check(lay, G, C, C, [], tag + ("verify clean",))
                X = C.copy()
                hit = _flip_some(lay, X, [1] * n, 2, 0, k)
                want = _ref_flags(lay, k, p, X)
                assert np.flatnonzero(want).tolist() == hit, tag  # the reference flags exactly the flipped objects
                d = Dev(lay, X)
                bad = d.flags()
                enc.verify_dev(d.base(), *_u(lay), bad, d.stream)
                CALLS[0] += 1
                G = d.result()
                assert bad.cpu().tolist() == want.tolist(), tag + ("verify flipped",)
                _check(lay, G, X, X, [], tag + ("verify flipped",))
            for e in range(1, p + 1):
                for ip, lost in enumerate(_patterns(k, p, e)):
                    present = [i not in lost for i in range(n)]
                    if "reconstruct" in ops:
                        for data_only in ((False, True) if ip == 0 else (False,)):
                            X = C.copy()
                            _garbage(lay, X, rng, lost)
                            W = X.copy()
                            written = _ref_reconstruct(lay, k, p, W, present, data_only)
                            d = Dev(lay, X)
                            enc.reconstruct_dev(d.base(), present, *_u(lay), data_only=data_only, stream=d.stream)
                            CALLS[0] += 1
                            _check(lay, d.result(), X, W, written, tag + ("reconstruct", lost, data_only))
                    if "decode" in ops and e < p and n <= 16:
                        for flipped in (False, True):
                            X = C.copy()
                            if flipped:
                                _flip_some(lay, X, present, 2, 0, k)
                            _garbage(lay, X, rng, lost)
                            W = X.copy()
                            written = _ref_reconstruct(lay, k, p, W, present)
                            want = _ref_flags(lay, k, p, W)  # Verify after Reconstruct on the same input
                            d = Dev(lay, X)
                            bad = d.flags()
                            enc.decode_dev(d.base(), present, *_u(lay), bad, d.stream)
                            CALLS[0] += 1
                            G = d.result()
                            assert bad.cpu().tolist() == want.tolist(), tag + ("decode", lost, flipped)
                            _check(lay, G, X, W, written, tag + ("decode", lost, flipped))


@gpu_test
@pytest.mark.parametrize("k", KS)
def test_uniform_every_form(gpu, k):
    sweep_uniform(k)


@gpu_test
@pytest.mark.parametrize("k", TWO_PASS_KS)
def test_uniform_two_passes(gpu, k):
    """p = 5..8: a pass of R = 4, then one of R = 1..4 with r0 = 4; ki applies
    to the last pass only (verify_dev, where k + p <= 16)."""
    sweep_uniform(k, ps=TWO_PASS_PS, shapes=(CHUNKS, SMALL), ops=("encode", "verify"))


# ------------------------------------------- section 4: the other families

def sweep_multi(k, ps=PS):
    """decode_dev_multi / reconstruct_dev_multi, every object its own pattern
    (cycled); shift 0: as the API routes an aligned batch; shift 8: the base
    is not 16-B aligned, which takes the host-planned gf_apply_multi launches."""
    for p in ps:
        n = k + p
        enc = _enc(k, p)
        pats = _multi_patterns(k, p)
        for shape in MULTI_SHAPES:
            lay = Uniform(n, *shape)
            rng = np.random.default_rng([k, p, *shape, 4])
            C = lay.host(rng)
            _ref_encode(lay, k, p, C)
            present = np.ones((lay.nobj, n), dtype=np.uint8)
            for o in range(lay.nobj):
                present[o, list(pats[o % len(pats)])] = 0
            for shift in (0, 8):
                for op in ("decode", "reconstruct", "data_only"):
                    tag = (k, p, shape, "multi", op, shift)
                    X = C.copy()
                    if op == "decode":
                        _flip_some(lay, X, present, 5, 0, k)
                    wr = np.zeros((lay.nobj, n), dtype=bool)
                    for o in range(lay.nobj):
                        _garbage(lay, X, rng, np.flatnonzero(present[o] == 0), [o])
                    W = X.copy()
                    for o in range(lay.nobj):
                        wr[o, _ref_reconstruct(lay, k, p, W, present[o], op == "data_only", [o])] = True
                    d = Dev(lay, X, shift)
                    if op == "decode":
                        want = _ref_flags(lay, k, p, W)
                        assert want.any() and not want.all(), tag  # the reference flags some objects, not all
                        bad = d.flags()
                        enc.decode_dev_multi(d.base(), present, *_u(lay), bad, d.stream)
                        G = d.result()
                        assert bad.cpu().tolist() == want.tolist(), tag
                    else:
                        enc.reconstruct_dev_multi(d.base(), present, *_u(lay), data_only=op == "data_only",
                                                  stream=d.stream)
                        G = d.result()
                    CALLS[0] += 1
                    _check(lay, G, X, W, wr, tag)


@gpu_test
@pytest.mark.parametrize("k", KS)
def test_multi_every_class(gpu, k):
    sweep_multi(k)


def sweep_var(k, ps=PS):
    """*_dev_objs: one call over objects of five sizes, each its own pitch,
    one of them corrupted.  A byte-packed object (pitch == S rounded up to 4)
    is outside these calls' contract (include/rsgpu.h: pitch >= shard_len
    rounded up to 16; objs_prepare): a table holding one is refused whole."""
    for p in ps:
        n = k + p
        enc = _enc(k, p)
        lay = Var(n, VAR_OBJS[:1] + (VAR_PACKED,) + VAR_OBJS[2:])
        X = lay.host(np.random.default_rng([k, p, 8]))
        d = Dev(lay, X)
        with pytest.raises(ia.InvalidArgument):
            enc.encode_dev_objs(d.objs(), d.stream)
        with pytest.raises(ia.InvalidArgument):
            enc.reconstruct_dev_objs(d.objs(), [False] + [True] * (n - 1), stream=d.stream)
        assert np.array_equal(d.result(), X), (k, p, "a refused call wrote")
        lay = Var(n, VAR_OBJS)
        rng = np.random.default_rng([k, p, 5])
        C = lay.host(rng)
        _ref_encode(lay, k, p, C)
        tag = (k, p, "objs")
        X = C.copy()
        _garbage(lay, X, rng, range(k, n))
        d = Dev(lay, X)
        enc.encode_dev_objs(d.objs(), d.stream)
        CALLS[0] += 1
        _check(lay, d.result(), X, C, range(k, n), tag + ("encode",))
        for e in range(1, p + 1):
            lost = _pattern_mixed(k, p, e)
            present = [i not in lost for i in range(n)]
            for data_only in (False, True):
                X = C.copy()
                _garbage(lay, X, rng, lost)
                W = X.copy()
                written = _ref_reconstruct(lay, k, p, W, present, data_only)
                d = Dev(lay, X)
                enc.reconstruct_dev_objs(d.objs(), present, data_only=data_only, stream=d.stream)
                CALLS[0] += 1
                _check(lay, d.result(), X, W, written, tag + ("reconstruct", lost, data_only))
        if n > 16:
            continue
        for hit in (None, (k + p) % lay.nobj):
            X = C.copy()
            if hit is not None:
                _flip(lay, X, hit, (hit * 3 + n - 1) % n, hit)
            want = [int(o == hit) for o in range(lay.nobj)]
            assert _ref_flags(lay, k, p, X).tolist() == want
            d = Dev(lay, X)
            bad = d.flags()
            enc.verify_dev_objs(d.objs(), bad, d.stream)
            CALLS[0] += 1
            G = d.result()
            assert bad.cpu().tolist() == want, tag + ("verify", hit)
            _check(lay, G, X, X, [], tag + ("verify", hit))
        for e in range(1, p):
            lost = _pattern_mixed(k, p, e)
            present = [i not in lost for i in range(n)]
            hit = (k + e) % lay.nobj
            X = C.copy()
            extra = [i for i in range(n) if present[i]][k:]
            _flip(lay, X, hit, extra[e % len(extra)], e)
            _garbage(lay, X, rng, lost)
            W = X.copy()
            written = _ref_reconstruct(lay, k, p, W, present)
            want = [int(o == hit) for o in range(lay.nobj)]
            assert _ref_flags(lay, k, p, W).tolist() == want
            d = Dev(lay, X)
            bad = d.flags()
            enc.decode_dev_objs(d.objs(), present, bad, d.stream)
            CALLS[0] += 1
            G = d.result()
            assert bad.cpu().tolist() == want, tag + ("decode", lost)
            _check(lay, G, X, W, written, tag + ("decode", lost))


@gpu_test
@pytest.mark.parametrize("k", KS)
def test_objs_every_class(gpu, k):
    sweep_var(k)


STATUS_TOO_FEW = 2  # include/rsgpu.h: fewer than data shards present, object untouched


def sweep_masks(k):
    """*_dev_masks for every p with k + p <= 16 (the masks API takes up to 32
    shards and returns not-implemented beyond: none in this grid, so every
    call here must succeed).  Rows and statuses against the reference."""
    import torch
    for p in PS:
        n = k + p
        if n > 16:
            continue
        enc = _enc(k, p)
        for shape in MASK_SHAPES:
            lay = Uniform(n, *shape)
            rng = np.random.default_rng([k, p, *shape, 6])
            C = lay.host(rng)
            _ref_encode(lay, k, p, C)
            present = _mask_present(k, p, shape[0], lay.nobj)
            few = [o for o in range(lay.nobj) if present[o].sum() < k]
            assert few and len(few) < lay.nobj
            masks = (present.astype(np.int64) << np.arange(n)).sum(axis=1).astype(np.uint32)
            dmasks = torch.from_numpy(masks.view(np.int32)).cuda()
            for op in ("decode", "reconstruct", "data_only"):
                tag = (k, p, shape, "masks", op)
                X = C.copy()
                if op == "decode":
                    _flip_some(lay, X, present, 2, 0, k)
                wr = np.zeros((lay.nobj, n), dtype=bool)
                for o in range(lay.nobj):
                    _garbage(lay, X, rng, np.flatnonzero(present[o] == 0), [o])
                W = X.copy()
                for o in range(lay.nobj):
                    if o not in few:
                        wr[o, _ref_reconstruct(lay, k, p, W, present[o], op == "data_only", [o])] = True
                want = _ref_flags(lay, k, p, W) if op == "decode" else np.zeros(lay.nobj, dtype=np.int32)
                want[few] = STATUS_TOO_FEW
                if op == "decode":  # the reference itself has every status the sweep is about
                    assert set(want.tolist()) == {0, 1, STATUS_TOO_FEW}, tag
                d = Dev(lay, X)
                status = d.flags(9)
                if op == "decode":
                    enc.decode_dev_masks(d.base(), dmasks, *_u(lay), status, d.stream)
                else:
                    enc.reconstruct_dev_masks(d.base(), dmasks, *_u(lay), data_only=op == "data_only", status=status,
                                              stream=d.stream)
                CALLS[0] += 1
                G = d.result()
                assert status.cpu().tolist() == want.tolist(), tag
                _check(lay, G, X, W, wr, tag)


@gpu_test
@pytest.mark.parametrize("k", KS[:-1])
def test_masks_every_class(gpu, k):
    sweep_masks(k)


@gpu_test
@pytest.mark.parametrize("k", KS)
def test_host_pinned_split_redirect(gpu, k):
    """Encode, Reconstruct and DecodeVerify (their C entry points, in place)
    on a pinned Split image: the pass reads and writes the caller's rows
    (kFormRedirect).  Every p = 1..4, so that Encode alone launches all 64
    instantiations; with k + p > 16 the fused decode's K passes kMaxK and
    takes the staged route, with the same results."""
    import ctypes
    from .test_gpu_random import _call_inplace
    S = HOST_S
    for p in PS:
        n = k + p
        enc = _enc(k, p)
        rng = np.random.default_rng([k, p, S])
        data = [rng.integers(0, 256, S, dtype=np.uint8) for _ in range(k)]
        e, full = oracle.encode(k, p, data + [bytes(S)] * p)
        assert e == 0
        assert np.array_equal(np.array(full[k:]), rn.apply(_matrix(k, p)[k:], data))
        host = ia.host_alloc(n * S)
        rows = [host[i * S:(i + 1) * S] for i in range(n)]
        for i in range(n):
            rows[i][:] = full[i] if i < k else rng.integers(0, 256, S, dtype=np.uint8)
        assert _call_inplace(enc, "rsgpu_encode", rows, [S] * n) == 0
        for i in range(n):
            assert np.array_equal(rows[i], full[i]), ("encode", k, p, i)
        for e_lost in sorted({1, p}):
            for flipped in (False, True):
                lost = _pattern_mixed(k, p, e_lost)
                for i in range(n):
                    rows[i][:] = full[i]
                if flipped:
                    present = [i for i in range(n) if i not in lost]
                    rows[present[-1]][S - 1] ^= 0x10
                ref = [None if i in lost else rows[i].copy() for i in range(n)]
                e, want = oracle.reconstruct(k, p, ref)
                assert e == 0
                e, want_ok = oracle.verify(k, p, want)
                assert e == 0
                lens = [0 if i in lost else S for i in range(n)]
                for fn in ("rsgpu_reconstruct", "rsgpu_decode"):
                    for i in lost:
                        rows[i][:] = rng.integers(0, 256, S, dtype=np.uint8)
                    if fn == "rsgpu_decode":
                        ok = ctypes.c_int(7)
                        assert _call_inplace(enc, fn, rows, lens, ctypes.byref(ok)) == 0
                        assert bool(ok.value) == want_ok, (fn, k, p, lost, flipped)
                    else:
                        assert _call_inplace(enc, fn, rows, lens, 0) == 0
                    for i in range(n):
                        assert np.array_equal(rows[i], want[i]), (fn, k, p, lost, flipped, i)


# ---------------------------- section 5: the kernels behind the env switches

def _child(which):
    """Runs in a fresh process with the switch set in its environment."""
    if which == "tri0":  # the six tri_shape()s fall back to launch_fixed / launch_fixed3
        sweep_uniform(10, ps=(3, 4), shapes=(CHUNKS,))
        sweep_uniform(12, ps=(4,), shapes=(CHUNKS,), ops=("verify",))
    elif which.startswith("staged0"):  # the staged shapes take kFormSmall, for every code
        for k in KS[int(which[-1])::2]:
            sweep_uniform(k, shapes=(STAGED, STAGED_EDGE))
    elif which == "triples2":  # storing passes of R >= 3 use Pass3
        for k in TRIPLE_KS:
            sweep_uniform(k, ps=(3, 4), ops=("encode", "decode"))
    elif which == "triples0":  # check-only passes of R >= 3 use single inputs
        for k in TRIPLE_KS:
            sweep_uniform(k, ps=(3, 4), ops=("verify",))
    else:
        raise SystemExit("unknown child " + which)
    assert CALLS[0] > 0
    print("forms child ok", which, CALLS[0])


_CHILD = "import sys; sys.path.insert(0, sys.argv[1]); from tests import test_gpu_forms as t; t._child(sys.argv[2])"


@gpu_test
@pytest.mark.parametrize("var,value,which", [("RSGPU_TRI", "0", "tri0"), ("RSGPU_STAGED", "0", "staged0-0"),
                                             ("RSGPU_STAGED", "0", "staged0-1"), ("RSGPU_TRIPLES", "2", "triples2"),
                                             ("RSGPU_TRIPLES", "0", "triples0")])
def test_fallback_kernels_behind_switches(gpu, var, value, which):
    env = dict(os.environ)
    env[var] = value
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, which], capture_output=True, text=True, timeout=300,
                       env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:] + r.stdout[-1000:]
    assert "forms child ok " + which in r.stdout


# ------------------------------------- the references agree (CPU, no device)

@pytest.mark.parametrize("k", KS)
def test_references_agree_on_every_pattern(k):
    """For every (k, p) of the grids and every loss pattern the sweeps use:
    rs_numpy.reconstruct, oracle.reconstruct and this file's batch reference
    give the same rows, and the inversion never reports singular; the parity
    of the two-pass codes agrees as well."""
    S = 19
    for p in PS + (TWO_PASS_PS if k in TWO_PASS_KS else ()):
        n = k + p
        rng = np.random.default_rng([k, p, 3])
        data = [rng.integers(0, 256, S, dtype=np.uint8) for _ in range(k)]
        e, full = oracle.encode(k, p, data + [bytes(S)] * p)
        assert e == 0
        assert np.array_equal(np.array(full[k:]), rn.encode(data, p)), (k, p)
        e, om = oracle.build_matrix(k, p)
        assert e == 0 and np.array_equal(om, _matrix(k, p)), (k, p)
        if p > 4:
            continue
        pats = {pat for e_lost in range(1, p + 1) for pat in _patterns(k, p, e_lost)}
        pats |= set(_multi_patterns(k, p))
        if n <= 16:
            for shape in MASK_SHAPES:
                for pr in _mask_present(k, p, shape[0], shape[2]):
                    if pr.sum() >= k:
                        pats.add(tuple(np.flatnonzero(pr == 0).tolist()))
        lay = Uniform(n, S, 32, 2)
        for lost in sorted(pats):
            for data_only in (False, True):
                shards = [None if i in lost else full[i].copy() for i in range(n)]
                e, want = oracle.reconstruct(k, p, shards, data_only=data_only)
                assert e == 0, (k, p, lost)  # never singular, never too few
                mine = rn.reconstruct(shards, k, p, data_only=data_only)
                A = lay.host(rng)
                for o in range(2):
                    for i in range(n):
                        if i not in lost:
                            lay.rows(A)[o][i, :S] = full[i]
                written = _ref_reconstruct(lay, k, p, A, [i not in lost for i in range(n)], data_only)
                assert written == [i for i in lost if i < k or not data_only]
                for i in range(n):
                    if i in lost and i >= k and data_only:
                        assert mine[i] is None
                        continue
                    assert np.array_equal(want[i], mine[i]), (k, p, lost, i)
                    assert np.array_equal(want[i], full[i]), (k, p, lost, i)
                    for o in range(2):
                        assert np.array_equal(lay.rows(A)[o][i, :S], want[i]), (k, p, lost, i, o)
