"""Per-object corrupted-shard location and repair on the device
(rsgpu_locate_dev_masks, rsgpu_repair_dev_masks): every object of a batch
brings its own present mask.  Bit for bit against numpy.

The reference is the statement of tests/test_gpu_locate.py (ref_locate,
restated here with the check matrices cached), applied per group of objects
sharing a mask; a mask the locator does not serve gives the code of the CPU
classification (tests/test_locate_masks_host.py classify).  After repair the
reference is the decode's own definition on the masks the locate wrote:
survivors = the first k present shards, missing rows = G[missing] x
inv(G[survivors]) x survivors, status 1 when a present row beyond the
survivors disagrees on [0, S), 2 with fewer than k present, 3 when the
survivors' matrix is singular (then nothing is written).  No tolerances."""
import functools
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import infinicache_amd as ia
from oracle import rs_numpy as rn
from tests.test_gpu_locate import _corrupt, _encoded, ref_locate
from tests.test_locate_masks_host import SINGULAR, TOO_FEW, TOO_MANY, classify

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLEAN, UNLOCATABLE = ia.LOC_CLEAN, ia.LOC_UNLOCATABLE


# ------------------------------------------------------------- the reference

@functools.lru_cache(maxsize=None)
def _matrix(k, p, kind):
    return rn.build_matrix(k, p, kind)


@functools.lru_cache(maxsize=None)
def _check_matrix(k, p, kind, mask):
    """H = [G[E] x inv(G[S]) | I_X] and order = S then E of the pattern."""
    G = _matrix(k, p, kind)
    Q = [i for i in range(k + p) if mask >> i & 1]
    S, E = Q[:k], Q[k:]
    C = rn.matmul(G[E], rn.invert(G[S]))
    return np.concatenate([C, np.eye(len(E), dtype=np.uint8)], axis=1), S + E


def _syndromes(H, order, rows, S):
    y = rows[:, order, :S]  # missing rows never read
    s = np.zeros((rows.shape[0], H.shape[0], S), dtype=np.uint8)
    for r in range(H.shape[0]):
        for q in range(H.shape[1]):
            if H[r, q]:
                s[:, r] ^= rn.MUL[H[r, q]][y[:, q]]
    return s


def ref_locate_mask(k, p, kind, mask, rows, S):
    """ref_locate of tests/test_gpu_locate.py for the objects `rows` sharing
    the served pattern `mask`: loc per object."""
    H, order = _check_matrix(k, p, kind, mask)
    X, w = H.shape
    s = _syndromes(H, order, rows, S)
    loc = np.full(rows.shape[0], CLEAN, dtype=np.int32)
    for o in np.flatnonzero(s.reshape(s.shape[0], -1).any(axis=1)):
        alive = [q for q in range(w)
                 if all((rn.MUL[H[b, q]][s[o, a]] == rn.MUL[H[a, q]][s[o, b]]).all()
                        for a, b in itertools.combinations(range(X), 2))]
        loc[o] = order[alive[0]] if len(alive) == 1 else UNLOCATABLE
    return loc


def reference(k, p, kind, masks, rows, S):
    """(loc, masks) of locate_dev_masks."""
    n = k + p
    cls = classify(k, p, kind)
    want_masks = (masks & np.uint32((1 << n) - 1)).astype(np.uint32)
    want_loc = np.empty(len(masks), dtype=np.int32)
    for m in np.unique(want_masks):
        idx = np.flatnonzero(want_masks == m)
        want_loc[idx] = cls[m] if cls[m] < 0 else ref_locate_mask(k, p, kind, int(m), rows[idx], S)
    for o in np.flatnonzero(want_loc >= 0):
        want_masks[o] &= ~np.uint32(1 << int(want_loc[o]))
    return want_loc, want_masks


def ref_decode(k, p, kind, masks, rows, S):
    """decode_dev_masks on `masks`: (status, rows afterwards; written rows
    are defined on [0, S) only)."""
    n = k + p
    G = _matrix(k, p, kind)
    status = np.zeros(len(masks), dtype=np.uint32)
    out = rows.copy()
    for m in np.unique(masks):
        idx = np.flatnonzero(masks == m)
        Q = [i for i in range(n) if int(m) >> i & 1]
        miss = [i for i in range(n) if i not in Q]
        if len(Q) < k:
            status[idx] = 2
            continue
        try:
            inv = rn.invert(G[Q[:k]])
        except rn.Singular:
            status[idx] = 3
            continue
        if miss:
            D = rn.matmul(G[miss], inv)
            for r, i in enumerate(miss):
                out[idx, i, :S] = 0
                for q in range(k):
                    if D[r, q]:
                        out[idx, i, :S] ^= rn.MUL[D[r, q]][rows[idx, Q[q], :S]]
        if len(Q) > k:
            H, order = _check_matrix(k, p, kind, int(m))
            status[idx] = _syndromes(H, order, rows[idx], S).reshape(len(idx), -1).any(axis=1)
    return status, out


# ------------------------------------------------------------------- batches

def _lost_mask(n, start, count):
    m = (1 << n) - 1
    for i in range(count):
        m &= ~(1 << ((start + i) % n))
    return m


def make_masks(k, p, nobj, rot, extra=()):
    """Masks cycling with the object index: all present; 1 .. p-2 lost at
    rotating positions (the first k included, so the survivors reach into
    parity); p-1 lost (TOO_FEW, yet decodable); p+1 lost (TOO_FEW, status 2);
    a served pattern with garbage in bits >= n; then `extra`.  Returns the
    masks and the cycle's period."""
    n = k + p
    kinds = [0] + list(range(1, p - 1)) + [p - 1, p + 1, "garbage"] + ["x%d" % i for i in range(len(extra))]
    masks = np.empty(nobj, dtype=np.uint32)
    for o in range(nobj):
        kind = kinds[o % len(kinds)]
        start = (o // len(kinds) * 3 + o + rot) % n
        if kind == "garbage":
            m = _lost_mask(n, start, max(0, p - 2)) | (0xABCDE << n)
        elif isinstance(kind, str):
            m = extra[int(kind[1:])]
        else:
            m = _lost_mask(n, start, kind)
        masks[o] = m & 0xFFFFFFFF
    return masks, len(kinds)


def corrupt(golden, masks, S, rot, rng, period):
    """The states of tests/test_gpu_locate.py's _corrupt, applied to each
    object's own present set: clean; one bit in the first byte / the last
    valid byte / a byte of the last 16-B vector; every present shard in turn
    randomised whole; two shards randomised; garbage in pad bytes only.
    Missing rows are 0xA5.  expected[o]: the single corrupted shard, CLEAN,
    or None (two shards)."""
    h = golden.copy()
    nobj, n, pitch = h.shape
    expected = []
    for o in range(nobj):
        Q = [i for i in range(n) if int(masks[o]) >> i & 1]
        h[o, [i for i in range(n) if i not in Q], :] = 0xA5
        nstate = 6 + len(Q)
        st = (o // period + o + rot) % nstate
        j = Q[(o * 7 + 3 + rot) % len(Q)]
        if st == 0:
            expected.append(CLEAN)
        elif st in (1, 2, 3):
            pos = 0 if st == 1 else S - 1 if st == 2 else (S - 1) // 16 * 16
            h[o, j, pos] ^= 1 << int(rng.integers(0, 8))
            expected.append(j)
        elif st == 4:
            a, b = (int(x) for x in rng.choice(Q, 2, replace=False))
            for i in (a, b):
                h[o, i, :S] ^= rng.integers(1, 256, S, dtype=np.uint8)
            expected.append(None)
        elif st == 5:
            h[o, Q[o % len(Q)], S:] = 0xEE  # (no pad bytes when pitch == S)
            h[o, Q[-1], S:] = 0x77
            expected.append(CLEAN)
        else:
            j = Q[st - 6]
            h[o, j, :S] ^= rng.integers(1, 256, S, dtype=np.uint8)  # every byte differs
            expected.append(j)
    return h, expected


def _dev_u32(a):
    return torch.from_numpy(a.view(np.int32).copy()).cuda()


def _host_u32(t):
    return t.cpu().numpy().view(np.uint32)


def _filled(nobj):
    return torch.full((nobj,), 77, dtype=torch.int32, device="cuda")


def run_case(k, p, kind, S, nobj, pitch, extra=()):
    """Two rounds on one context (other masks and corruption, a non-default
    stream: the scratch must have reset itself).  Returns what the device
    calls left, for comparisons between launch forms."""
    n = k + p
    stride = n * pitch
    enc = ia.New(k, p, matrix=kind)
    cls = classify(k, p, kind)
    rng = np.random.default_rng(S * 1000 + nobj + n)
    b, golden = _encoded(enc, n, S, pitch, nobj, seed=S + nobj + n)
    side = torch.cuda.Stream()
    left = {}
    for rnd, (rot, stream) in enumerate(((S + nobj, torch.cuda.current_stream()), (S + nobj + 5, side))):
        masks_np, period = make_masks(k, p, nobj, rot, extra)
        h, expected = corrupt(golden, masks_np, S, rot, rng, period)
        want_loc, want_masks = reference(k, p, kind, masks_np, h, S)
        trunc = masks_np & np.uint32((1 << n) - 1)
        served = cls[trunc] >= 0
        assert np.array_equal(want_loc[~served], cls[trunc][~served])
        if kind != "par1":  # MDS: one corrupted shard is always named, clean never flagged
            for o in np.flatnonzero(served):
                e = expected[o]
                if e is not None:
                    assert want_loc[o] == e, (o, e, want_loc[o])
                elif S >= 16:
                    assert want_loc[o] == UNLOCATABLE, o
        print(kind, k, p, S, nobj, "round", rnd, "served", int(served.sum()), "located", int((want_loc >= 0).sum()),
              "unlocatable", int((want_loc == UNLOCATABLE).sum()),
              "codes", {c: int((want_loc == c).sum()) for c in (TOO_FEW, TOO_MANY, SINGULAR)})
        b.copy_(torch.from_numpy(h))
        present = _dev_u32(masks_np)
        loc, masks = _filled(nobj), _filled(nobj)
        torch.cuda.synchronize()
        enc.locate_dev_masks(b, present, S, pitch, stride, nobj, loc, masks, stream)
        stream.synchronize()
        assert np.array_equal(loc.cpu().numpy(), want_loc)
        assert np.array_equal(_host_u32(masks), want_masks)
        assert np.array_equal(b.cpu().numpy(), h)  # locate writes nothing to the rows
        assert np.array_equal(_host_u32(present), masks_np)
        # without the optional masks
        loc.fill_(77)
        torch.cuda.synchronize()
        enc.locate_dev_masks(b, present, S, pitch, stride, nobj, loc, None, stream)
        stream.synchronize()
        assert np.array_equal(loc.cpu().numpy(), want_loc)
        # in place
        loc.fill_(77)
        inplace = present.clone()
        torch.cuda.synchronize()
        enc.locate_dev_masks(b, inplace, S, pitch, stride, nobj, loc, inplace, stream)
        stream.synchronize()
        assert np.array_equal(loc.cpu().numpy(), want_loc)
        assert np.array_equal(_host_u32(inplace), want_masks)

        # repair: the locate, then the masked decode on the masks it wrote
        want_status, want_rows = ref_decode(k, p, kind, want_masks, h, S)
        loc.fill_(77)
        masks.fill_(77)
        status = _filled(nobj)
        torch.cuda.synchronize()
        enc.repair_dev_masks(b, present, S, pitch, stride, nobj, loc, masks, status, stream)
        stream.synchronize()
        got, st = b.cpu().numpy(), _host_u32(status)
        assert np.array_equal(loc.cpu().numpy(), want_loc)
        assert np.array_equal(_host_u32(masks), want_masks)
        assert np.array_equal(st, want_status), np.flatnonzero(st != want_status)[:8]
        for o in range(nobj):
            Q = [i for i in range(n) if int(want_masks[o]) >> i & 1]
            assert np.array_equal(got[o, Q], h[o, Q]), o  # rows the decode takes as present: untouched
            assert np.array_equal(got[o, :, :S], want_rows[o, :, :S]), (o, want_loc[o])
            if st[o] >= 2:
                assert np.array_equal(got[o], h[o]), o  # nothing written at all
            if want_loc[o] == UNLOCATABLE:
                assert st[o] == 1, o
            elif want_loc[o] == CLEAN or (want_loc[o] >= 0 and expected[o] is not None and kind != "par1"):
                # good or healed: the golden rows on [0, S)
                assert st[o] == 0, (o, want_loc[o])
                assert np.array_equal(got[o, :, :S], golden[o, :, :S]), (o, want_loc[o])
            elif want_loc[o] >= 0 and expected[o] is None:
                # two shards randomised in a very short object can look like one bad shard elsewhere
                assert S < 16 or kind == "par1", o
        left["loc%d" % rnd], left["masks%d" % rnd], left["status%d" % rnd] = loc.cpu().numpy(), _host_u32(masks), st
        left["rows%d" % rnd] = got[:, :, :S].copy()
    return left


def _p16(S):
    return (S + 15) // 16 * 16


RS104 = (10, 4, "vandermonde")
LONG = {
    "long-2049": RS104 + (2049, 40, _p16(2049)),        # first long size: 129 vectors
    "long-4097": RS104 + (4097, 40, 4352),              # two chunks, 1-byte tail, pitch rounded to 256
    "long-12292": RS104 + (12292, 3, _p16(12292)),
    "one-147": RS104 + (147, 1, 160),                   # nobj = 1: the long-row form on a short row
}
SHORT = {
    "short-1": RS104 + (1, 257, 16),
    "short-103": RS104 + (103, 77, 112),                # nvec 7, opw 36, ragged last group
    "short-147": RS104 + (147, 57, 160),                # nvec 10: objects straddle waves
    "short-2048": RS104 + (2048, 5, 2048),              # nvec 128, opw 2: the boundary
}
OTHER = {}
for _name, _code, _extra in (("rs6+3", (6, 3, "vandermonde"), ()), ("rs4+6", (4, 6, "vandermonde"), ()),
                             ("rs10+2", (10, 2, "vandermonde"), ()), ("cauchy10+4", (10, 4, "cauchy"), ()),
                             ("par1-5+6", (5, 6, "par1"), (0x766, 0x778))):
    for _S, _nobj, _pitch in ((15, 257, 16), (147, 57, 160), (4097, 40, 4352)):
        OTHER["%s-%d" % (_name, _S)] = _code + (_S, _nobj, _pitch, _extra)
CASES = {**LONG, **SHORT, **OTHER}
_LEFT = {}


def _left(name):
    if name not in _LEFT:
        _LEFT[name] = run_case(*CASES[name])
    return _LEFT[name]


@pytest.mark.parametrize("name", list(CASES))
def test_locate_and_repair_dev_masks(gpu, name):
    _left(name)


def test_batch_reaches_every_code():
    """The batches above hold what they are meant to hold."""
    cls = classify(4, 6, "vandermonde")
    m, _ = make_masks(4, 6, 57, 0)
    got = set(cls[m & 0x3FF].tolist())
    assert {TOO_MANY, TOO_FEW, 2, 3, 4} <= got
    cls = classify(5, 6, "par1")
    m, _ = make_masks(5, 6, 57, 0, (0x766, 0x778))
    assert SINGULAR in set(cls[m & 0x7FF].tolist())
    cls = classify(10, 4, "vandermonde")
    m, _ = make_masks(10, 4, 40, 0)
    assert {TOO_FEW, 2, 3, 4} <= set(cls[m & 0x3FFF].tolist())
    assert (m >> 14).any() and (m & 0x3FF != 0x3FF).any()  # garbage bits; survivors reaching into parity


_CHILD = ("import sys; sys.path.insert(0, sys.argv[1]); import numpy as np; "
          "import tests.test_gpu_locate_masks as t; "
          "np.savez(sys.argv[2], **{n + '/' + k: v for n in t.SHORT for k, v in t.run_case(*t.SHORT[n]).items()})")


def test_short_rows_long_form_agrees(gpu, tmp_path):
    """Every short-row shape once more in a fresh process with the short-row
    form switched off (RSGPU_LOCATE_LANES=0 is read at load): the same checks
    pass there and both forms leave identical words and rows."""
    out = str(tmp_path / "long_form.npz")
    env = dict(os.environ, RSGPU_LOCATE_LANES="0")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, out], capture_output=True, text=True, timeout=300,
                       env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    other = np.load(out)
    for name in SHORT:
        mine = _left(name)
        for key, val in mine.items():
            assert np.array_equal(other[name + "/" + key], val), (name, key)


# ------------------------------------------------- agreement with locate_dev

@pytest.mark.parametrize("S,pitch", [(147, 160), (4097, 4112)])
@pytest.mark.parametrize("lost", [(), (0, 5)])
def test_uniform_batch_equals_locate_dev(gpu, lost, S, pitch):
    k, p, nobj = 10, 4, 40
    n = k + p
    present = [i not in lost for i in range(n)]
    pm = sum(1 << i for i in range(n) if present[i])
    enc = ia.New(k, p)
    rng = np.random.default_rng(S + len(lost))
    b, golden = _encoded(enc, n, S, pitch, nobj, seed=S + 5)
    h, _ = _corrupt(golden, present, S, 2, rng)
    b.copy_(torch.from_numpy(h))
    loc_u, masks_u, loc_m, masks_m = (_filled(nobj) for _ in range(4))
    torch.cuda.synchronize()
    enc.locate_dev(b, present, S, pitch, n * pitch, nobj, loc_u, masks_u)
    enc.locate_dev_masks(b, _dev_u32(np.full(nobj, pm, dtype=np.uint32)), S, pitch, n * pitch, nobj, loc_m, masks_m)
    torch.cuda.synchronize()
    want_loc, want_masks = ref_locate(k, p, "vandermonde", present, h, S)
    assert (want_loc >= 0).any() and (want_loc == UNLOCATABLE).any() and (want_loc == CLEAN).any()
    assert np.array_equal(loc_u.cpu().numpy(), want_loc)
    assert np.array_equal(loc_m.cpu().numpy(), loc_u.cpu().numpy())
    assert np.array_equal(masks_m.cpu().numpy(), masks_u.cpu().numpy())


def test_no_objects(gpu):
    enc = ia.New(10, 4)
    b = torch.zeros(14 * 16, dtype=torch.uint8, device="cuda")
    enc.locate_dev_masks(b, None, 16, 16, 14 * 16, 0, None, None)
    enc.repair_dev_masks(b, None, 16, 16, 14 * 16, 0, None, None, None)
    torch.cuda.synchronize()


def test_multi_device_context_routes_by_owner(gpu):
    """A context over a repeated device: the calls go to an entry that owns
    d_base (each entry uploads its own copy of the shared host table) and
    give what a single-device context gives."""
    k, p, kind, S, nobj, pitch = RS104 + (147, 57, 160)
    n = k + p
    enc = ia.New(k, p, devices=[0, 0])
    assert enc.locate_pattern(0x3FFF) == 4 and enc.locate_pattern(0x3FF) == TOO_FEW
    b, golden = _encoded(ia.New(k, p), n, S, pitch, nobj, seed=9)
    masks_np, period = make_masks(k, p, nobj, 2)
    h, _ = corrupt(golden, masks_np, S, 2, np.random.default_rng(5), period)
    want_loc, want_masks = reference(k, p, kind, masks_np, h, S)
    want_status, want_rows = ref_decode(k, p, kind, want_masks, h, S)
    present = _dev_u32(masks_np)
    base = enc.device_calls()
    for _ in range(2):  # round-robin over the two entries
        b.copy_(torch.from_numpy(h))
        loc, masks, status = _filled(nobj), _filled(nobj), _filled(nobj)
        enc.repair_dev_masks(b, present, S, pitch, n * pitch, nobj, loc, masks, status)
        torch.cuda.synchronize()
        assert np.array_equal(loc.cpu().numpy(), want_loc)
        assert np.array_equal(_host_u32(masks), want_masks)
        assert np.array_equal(_host_u32(status), want_status)
        assert np.array_equal(b.cpu().numpy()[:, :, :S], want_rows[:, :, :S])
    assert all(c > b0 for c, b0 in zip(enc.device_calls(), base)), (enc.device_calls(), base)


# ------------------------------------------------------------ shard-major

@pytest.mark.parametrize("S,stride", [(1000, 1008), (3000, 3008)])
def test_locate_masks_shard_major_layout(gpu, S, stride):
    """[shard][object]: every shard row holds each object's piece; two
    different masks in the batch."""
    k, p, nobj = 10, 4, 9
    n = k + p
    pitch = (nobj * stride + 255) // 256 * 256
    enc = ia.New(k, p)
    g = torch.Generator(device="cuda").manual_seed(3)
    b = torch.randint(0, 256, (n, pitch), dtype=torch.uint8, device="cuda", generator=g)
    enc.encode_dev(b, S, pitch, stride, nobj, torch.cuda.current_stream())
    torch.cuda.synchronize()
    h = b.cpu().numpy()
    masks_np = np.array([0x3FFF if o % 2 == 0 else 0x3FFF & ~0x21 for o in range(nobj)], dtype=np.uint32)
    for o in range(1, nobj, 2):  # the pieces that did not arrive
        h[[0, 5], o * stride:(o + 1) * stride] = 0xA5
    h[4, 3 * stride + S - 1] ^= 0x10     # object 3 ({0,5} lost), shard 4, last valid byte
    h[11, 6 * stride + 0] ^= 0x01        # object 6 (all present), shard 11
    h[0, 2 * stride + 17] ^= 0x80        # object 2 (all present), shard 0
    h[2, 5 * stride + S:5 * stride + stride] ^= 0xFF  # gap bytes of object 5: pads
    rows = np.stack([h[:, o * stride:o * stride + stride] for o in range(nobj)])
    want_loc, want_masks = reference(k, p, "vandermonde", masks_np, rows, S)
    assert want_loc.tolist() == [CLEAN, CLEAN, 0, 4, CLEAN, CLEAN, 11, CLEAN, CLEAN]
    b.copy_(torch.from_numpy(h))
    loc, masks = _filled(nobj), _filled(nobj)
    enc.locate_dev_masks(b, _dev_u32(masks_np), S, pitch, stride, nobj, loc, masks)
    torch.cuda.synchronize()
    assert np.array_equal(loc.cpu().numpy(), want_loc)
    assert np.array_equal(_host_u32(masks), want_masks)
    assert np.array_equal(b.cpu().numpy(), h)


# ---------------------------------------------------------------------- graph

@pytest.mark.parametrize("S,pitch,nobj", [(147, 160, 57), (4097, 4112, 40)])
def test_capture_locate_masks_then_decode(gpu, S, pitch, nobj):
    """After a first eager call, locate_dev_masks + decode_dev_masks on one
    stream capture into a single chain; replays on other masks and freshly
    corrupted data written into the same buffers."""
    k, p, kind = 10, 4, "vandermonde"
    n = k + p
    stride = n * pitch
    enc = ia.New(k, p)
    rng = np.random.default_rng(11)
    b, golden = _encoded(enc, n, S, pitch, nobj, seed=21)
    present = torch.zeros(nobj, dtype=torch.int32, device="cuda")
    present.fill_(0x3FFF)
    loc, masks, status = (torch.zeros(nobj, dtype=torch.int32, device="cuda") for _ in range(3))
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        enc.locate_dev_masks(b, present, S, pitch, stride, nobj, loc, masks, st)  # tables: outside the capture
        enc.decode_dev_masks(b, masks, S, pitch, stride, nobj, status, st)
    st.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=st):
        enc.locate_dev_masks(b, present, S, pitch, stride, nobj, loc, masks, st)
        enc.decode_dev_masks(b, masks, S, pitch, stride, nobj, status, st)
    for rep in range(2):
        masks_np, period = make_masks(k, p, nobj, rep * 4 + 1)
        h, _ = corrupt(golden, masks_np, S, rep * 3 + 1, rng, period)
        want_loc, want_masks = reference(k, p, kind, masks_np, h, S)
        want_status, want_rows = ref_decode(k, p, kind, want_masks, h, S)
        assert (want_loc >= 0).any() and (want_loc == TOO_FEW).any() and (want_status == 2).any()
        b.copy_(torch.from_numpy(h))
        present.copy_(_dev_u32(masks_np))
        loc.fill_(77)
        masks.fill_(77)
        status.fill_(77)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(loc.cpu().numpy(), want_loc), rep
        assert np.array_equal(_host_u32(masks), want_masks), rep
        assert np.array_equal(_host_u32(status), want_status), rep
        assert np.array_equal(b.cpu().numpy()[:, :, :S], want_rows[:, :, :S]), rep
