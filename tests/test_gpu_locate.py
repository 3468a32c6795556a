"""Corrupted-shard location and repair on the device (rsgpu_locate_dev,
rsgpu_repair_dev, rsgpu_locate, rsgpu_repair, Client(repair=True)) against a
numpy statement of the definition in include/rsgpu.h, bit for bit.

Reference, per erasure pattern: Q = present shards in index order, S = the
first k, E = the rest, H = [G[E] x inv(G[S]) | I_X] over the columns S then E;
s(c) = H x y(c) for every byte column c < shard_len.  clean: every s(c) zero;
column position q alive: H[b][q] * s_a(c) == H[a][q] * s_b(c) for every c and
row pair a < b; located at order[q] when not clean and exactly one position is
alive; unlocatable otherwise."""
import itertools

import numpy as np
import pytest

import infinicache_amd as ia
from oracle import rs_numpy as rn

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CLEAN, UNLOCATABLE = ia.LOC_CLEAN, ia.LOC_UNLOCATABLE


# ------------------------------------------------------------- the reference

def ref_check_matrix(k, p, kind, present):
    G = rn.build_matrix(k, p, kind)
    Q = [i for i in range(k + p) if present[i]]
    S, E = Q[:k], Q[k:]
    C = rn.matmul(G[E], rn.invert(G[S]))
    return np.concatenate([C, np.eye(len(E), dtype=np.uint8)], axis=1), S + E


def ref_locate(k, p, kind, present, rows, S):
    """rows: (nobj, k+p, >= S) uint8.  Returns (loc, masks) per object."""
    H, order = ref_check_matrix(k, p, kind, present)
    X, w = H.shape
    y = rows[:, order, :S]                                    # (nobj, w, S): missing rows never read
    s = np.zeros((rows.shape[0], X, S), dtype=np.uint8)
    for r in range(X):
        for q in range(w):
            if H[r, q]:
                s[:, r] ^= rn.MUL[H[r, q]][y[:, q]]
    dirty = s.reshape(s.shape[0], -1).any(axis=1)
    alive = np.ones((rows.shape[0], w), dtype=bool)
    for q in range(w):
        for a, b in itertools.combinations(range(X), 2):
            alive[:, q] &= (rn.MUL[H[b, q]][s[:, a]] == rn.MUL[H[a, q]][s[:, b]]).all(axis=1)
    pm = sum(1 << i for i in range(k + p) if present[i])
    loc = np.full(rows.shape[0], CLEAN, dtype=np.int32)
    masks = np.full(rows.shape[0], pm, dtype=np.uint32)
    for o in np.flatnonzero(dirty):
        loc[o] = UNLOCATABLE
        if alive[o].sum() == 1:
            loc[o] = order[int(np.flatnonzero(alive[o])[0])]
            masks[o] = pm & ~(1 << int(loc[o]))
    return loc, masks


# ------------------------------------------------------------------- batches

def _encoded(enc, n, S, pitch, nobj, seed):
    """nobj encoded objects [object][shard][pitch], zero pad bytes: (device, host)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    b = torch.randint(0, 256, (nobj, n, pitch), dtype=torch.uint8, device="cuda", generator=g)
    b[:, :, S:] = 0
    enc.encode_dev(b, S, pitch, n * pitch, nobj, torch.cuda.current_stream())
    torch.cuda.synchronize()
    return b, b.cpu().numpy()


def _corrupt(golden, present, S, rot, rng):
    """Per-object states, cycling with the object index: clean; one bit in the
    first byte / the last valid byte / a byte of the last 16-B vector; every
    present shard in turn randomised whole; two shards randomised; garbage in
    pad bytes only.  Missing rows are 0xA5.  Returns (rows, expected) where
    expected[o] is the single corrupted shard, CLEAN, or None (two shards)."""
    h = golden.copy()
    nobj, n, pitch = h.shape
    Q = [i for i in range(n) if present[i]]
    lost = [i for i in range(n) if not present[i]]
    h[:, lost, :] = 0xA5
    nstate = 6 + len(Q)
    expected = []
    for o in range(nobj):
        st = (o + rot) % nstate
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


CODES = {
    "rs10+2": (10, 2, "vandermonde", ()),
    "rs10+4-2lost": (10, 4, "vandermonde", (0, 5)),
    "rs10+4": (10, 4, "vandermonde", ()),
    "rs6+3": (6, 3, "vandermonde", ()),
    "rs6+3-1lost": (6, 3, "vandermonde", (2,)),
    "rs4+2": (4, 2, "vandermonde", ()),
    "cauchy10+2": (10, 2, "cauchy", ()),
    "par1-10+4-2lost": (10, 4, "par1", (0, 5)),
}

LENS = (1, 15, 16, 17, 4095, 4096, 4097, 12289 + 3)  # the last: 4 chunks of 256 lanes x 16 B

CASES = [("rs10+2", S, 3, False) for S in LENS]
CASES += [("rs10+2", 17, 257, False), ("rs10+2", 4097, 257, False), ("rs10+2", 12289 + 3, 1, False),
          ("rs10+2", 4097, 3, True), ("rs10+2", 1, 257, False), ("rs10+2", 16, 1, False)]
for _code in list(CODES)[1:]:
    CASES += [(_code, 15, 257, False), (_code, 4097, 40, True), (_code, 12289 + 3, 3, False), (_code, 4096, 1, False)]


@pytest.mark.parametrize("code,S,nobj,pitch256", CASES)
def test_locate_and_repair_dev(gpu, code, S, nobj, pitch256):
    k, p, kind, lost = CODES[code]
    n = k + p
    present = [i not in lost for i in range(n)]
    pitch = (S + 255) // 256 * 256 if pitch256 else (S + 15) // 16 * 16
    stride = n * pitch
    enc = ia.New(k, p, matrix=kind)
    rng = np.random.default_rng(S * 1000 + nobj + n)
    b, golden = _encoded(enc, n, S, pitch, nobj, seed=S + nobj + n)
    side = torch.cuda.Stream()
    for rot, stream in ((S + nobj, torch.cuda.current_stream()), (S + nobj + 5, side)):
        # (the second round: other corruption on the same context, so the
        # scratch must have reset itself; and a non-default stream)
        h, expected = _corrupt(golden, present, S, rot, rng)
        want_loc, want_masks = ref_locate(k, p, kind, present, h, S)
        if kind != "par1":  # MDS: one corrupted shard is always named, clean never flagged
            for o, e in enumerate(expected):
                if e is not None:
                    assert want_loc[o] == e, (o, e, want_loc[o])
                elif S >= 16:
                    assert want_loc[o] == UNLOCATABLE, o
        b.copy_(torch.from_numpy(h))
        loc = torch.full((nobj,), 77, dtype=torch.int32, device="cuda")
        masks = torch.full((nobj,), 77, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        enc.locate_dev(b, present, S, pitch, stride, nobj, loc, masks, stream)
        stream.synchronize()
        print(code, S, nobj, "located", int((want_loc >= 0).sum()), "unlocatable", int((want_loc == UNLOCATABLE).sum()))
        assert np.array_equal(loc.cpu().numpy(), want_loc)
        assert np.array_equal(masks.cpu().numpy().view(np.uint32), want_masks)
        assert np.array_equal(b.cpu().numpy(), h)  # locate writes nothing
        # without the optional masks
        loc.fill_(77)
        torch.cuda.synchronize()
        enc.locate_dev(b, present, S, pitch, stride, nobj, loc, None, stream)
        stream.synchronize()
        assert np.array_equal(loc.cpu().numpy(), want_loc)

        # repair: locate, then the masked decode on the masks it wrote
        loc.fill_(77)
        masks.fill_(77)
        status = torch.full((nobj,), 77, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        enc.repair_dev(b, present, S, pitch, stride, nobj, loc, masks, status, stream)
        stream.synchronize()
        got, st = b.cpu().numpy(), status.cpu().numpy()
        assert np.array_equal(loc.cpu().numpy(), want_loc)
        assert np.array_equal(masks.cpu().numpy().view(np.uint32), want_masks)
        Q = [i for i in range(n) if present[i]]
        for o in range(nobj):
            if want_loc[o] == UNLOCATABLE:
                assert st[o] == 1, o
                assert np.array_equal(got[o, Q], h[o, Q]), o  # present rows untouched
            elif expected[o] is None:
                # two shards randomised in a very short object can look like one
                # bad shard elsewhere: "healed" to something consistent, not to the original
                assert S < 16 or kind == "par1", o
            elif kind != "par1" or st[o] == 0:
                assert st[o] == 0, (o, want_loc[o])
                assert np.array_equal(got[o, :, :S], golden[o, :, :S]), (o, want_loc[o])
            else:  # PAR1: the pattern without the located shard may be singular (3) or ambiguous (1)
                assert st[o] in (1, 3), o


def test_locate_shard_major_layout(gpu):
    """[shard][object]: every shard row holds each object's piece."""
    k, p, S, nobj = 10, 2, 1000, 9
    n = k + p
    stride = 1008
    pitch = (nobj * stride + 255) // 256 * 256
    enc = ia.New(k, p)
    g = torch.Generator(device="cuda").manual_seed(3)
    b = torch.randint(0, 256, (n, pitch), dtype=torch.uint8, device="cuda", generator=g)
    enc.encode_dev(b, S, pitch, stride, nobj, torch.cuda.current_stream())
    torch.cuda.synchronize()
    h = b.cpu().numpy()
    h[4, 3 * stride + 999] ^= 0x10      # object 3, shard 4, last valid byte
    h[11, 7 * stride + 0] ^= 0x01       # object 7, shard 11
    h[2, 5 * stride + 1000:5 * stride + 1008] ^= 0xFF  # gap bytes of object 5: pads
    rows = np.stack([h[:, o * stride:o * stride + stride] for o in range(nobj)])
    want_loc, want_masks = ref_locate(k, p, "vandermonde", [1] * n, rows, S)
    assert want_loc.tolist() == [CLEAN] * 3 + [4] + [CLEAN] * 3 + [11, CLEAN]
    b.copy_(torch.from_numpy(h))
    loc = torch.full((nobj,), 77, dtype=torch.int32, device="cuda")
    masks = torch.full((nobj,), 77, dtype=torch.int32, device="cuda")
    enc.locate_dev(b, [1] * n, S, pitch, stride, nobj, loc, masks)
    torch.cuda.synchronize()
    assert np.array_equal(loc.cpu().numpy(), want_loc)
    assert np.array_equal(masks.cpu().numpy().view(np.uint32), want_masks)


# ---------------------------------------------------------------- host shards

@pytest.mark.parametrize("k,p,lost", [(10, 4, (0, 5)), (10, 2, ()), (6, 3, (7,))])
def test_locate_and_repair_host_shards(gpu, k, p, lost):
    n = k + p
    enc = ia.New(k, p)
    obj = rn.splitmix64_bytes(0x10CA7E, k, 10 * 1000 + 3)
    good = enc.Split(obj)
    enc.Encode(good)
    good = [s.copy() for s in good]

    def arrived():
        return [None if i in lost else good[i].copy() for i in range(n)]

    # clean
    sh = arrived()
    assert enc.Locate(sh) == CLEAN
    assert enc.Repair(sh) == (CLEAN, True)
    assert all(np.array_equal(sh[i], good[i]) for i in range(n))
    # one corrupted shard: a survivor, then an extra
    present = [i for i in range(n) if i not in lost]
    for bad in (present[1], present[-1]):
        sh = arrived()
        sh[bad][len(sh[bad]) - 1] ^= 0x40
        keep = list(sh)
        before = [None if s is None else s.copy() for s in sh]
        assert enc.Locate(sh) == bad
        assert all(s is None if b is None else np.array_equal(s, b) for s, b in zip(sh, before))  # Locate writes nothing
        assert enc.Repair(sh) == (bad, True)
        assert all(np.array_equal(sh[i], good[i]) for i in range(n))
        assert all(sh[i] is keep[i] for i in present)  # healed in the caller's buffer
    # two corrupted shards: nothing to name; the present shards stay as they came
    sh = arrived()
    sh[present[0]][0] ^= 1
    sh[present[3]][7] ^= 2
    before = [None if s is None else s.copy() for s in sh]
    assert enc.Locate(sh) == UNLOCATABLE
    assert enc.Repair(sh) == (UNLOCATABLE, False)
    assert all(np.array_equal(sh[i], before[i]) for i in present)
    assert all(sh[i] is not None and len(sh[i]) == len(good[0]) for i in lost)  # filled, as Reconstruct
    # bytearray shards (what the client holds)
    sh = [None if s is None else bytearray(s.tobytes()) for s in arrived()]
    sh[present[2]][5] ^= 0x80
    assert enc.Repair(sh) == (present[2], True)
    assert all(bytes(sh[i]) == good[i].tobytes() for i in range(n))


# --------------------------------------------------------------------- client

def test_client_get_repairs_over_proxy(gpu):
    from infinicache_amd.client import Client
    from tests.fake_proxy import FakeProxy

    proxy = FakeProxy()
    proxy.force_late = {0, 5}  # config 3's Get: 12 of 14 arrive
    val = rn.splitmix64_bytes(0xC11E, 1, 200_003).tobytes()
    try:
        for repair in (True, False):
            c = Client(10, 4, 0, device=0, repair=repair)
            assert c.Dial([proxy.addr])
            key = "obj-%d" % repair
            assert c.EcSet(key, val)[1]
            stored = {i: proxy.store[(key, str(i))] for i in range(14)}
            inner_get, recovered = c.get, []

            def flipping_get(addr, key, i, reqId, ret, inner_get=inner_get):
                inner_get(addr, key, i, reqId, ret)
                if i == 8 and ret.Ret(i) is not None:  # silently corrupted on its way back
                    body = bytearray(ret.Ret(i))
                    body[len(body) // 2] ^= 0x04
                    ret.Set(i, bytes(body))

            inner_recover = c.recover

            def recording_recover(addr, key, reqId, shards, failed, inner_recover=inner_recover):
                recovered.append(list(failed))
                inner_recover(addr, key, reqId, shards, failed)

            c.get, c.recover = flipping_get, recording_recover
            sets = proxy.sets
            _, reader, ok = c.EcGet(key, len(val))
            if repair:
                assert ok and reader.read() == val
                assert c.Data.Repaired == 8
                assert recovered == [[8]] and proxy.sets == sets + 1
                assert proxy.store[(key, "8")] == stored[8]  # the healed chunk was re-Set
            else:  # as today: the Get is lost
                assert not ok and reader is None
                assert recovered == [] and proxy.sets == sets and c.Data.Repaired is None
            c.Close()
    finally:
        proxy.close()


# ---------------------------------------------------------------------- graph

def test_capture_locate_then_decode(gpu):
    """After a first eager call, locate_dev + decode_dev_masks on one stream
    capture into a (linear) graph; replays on freshly corrupted data."""
    k, p, S, nobj = 10, 4, 4099, 60
    n = k + p
    lost = (0, 5)
    present = [i not in lost for i in range(n)]
    pitch = (S + 15) // 16 * 16
    stride = n * pitch
    enc = ia.New(k, p)
    rng = np.random.default_rng(11)
    b, golden = _encoded(enc, n, S, pitch, nobj, seed=21)
    loc = torch.zeros(nobj, dtype=torch.int32, device="cuda")
    masks = torch.zeros(nobj, dtype=torch.int32, device="cuda")
    status = torch.zeros(nobj, dtype=torch.int32, device="cuda")
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        enc.locate_dev(b, present, S, pitch, stride, nobj, loc, masks, st)  # plans, atlas: outside the capture
        enc.decode_dev_masks(b, masks, S, pitch, stride, nobj, status, st)
    st.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=st):
        enc.locate_dev(b, present, S, pitch, stride, nobj, loc, masks, st)
        enc.decode_dev_masks(b, masks, S, pitch, stride, nobj, status, st)
    for rep in range(2):
        h, _ = _corrupt(golden, present, S, rep * 3 + 1, rng)
        want_loc, want_masks = ref_locate(k, p, "vandermonde", present, h, S)
        b.copy_(torch.from_numpy(h))
        loc.fill_(77)
        status.fill_(77)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(loc.cpu().numpy(), want_loc), rep
        assert np.array_equal(masks.cpu().numpy().view(np.uint32), want_masks), rep
        got, stat = b.cpu().numpy(), status.cpu().numpy()
        for o in range(nobj):
            assert stat[o] == (1 if want_loc[o] == UNLOCATABLE else 0), (rep, o)
            if want_loc[o] != UNLOCATABLE:
                assert np.array_equal(got[o, :, :S], golden[o, :, :S]), (rep, o)
