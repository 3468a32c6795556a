"""Corrupted-shard location, the parts that need no GPU: rsgpu_check_matrix
against a numpy H / order built from the oracle's matrices, the error table
of include/rsgpu.h (returned before any device is touched), and
Client.decode's repair step with a stub codec."""
import ctypes
import io
import itertools

import numpy as np
import pytest

import infinicache_amd as ia
from infinicache_amd import _lib
from infinicache_amd.client import Client, DataEntry
from oracle import rs_numpy as rn


def ref_check_matrix(k, p, kind, present):
    """H = [G[E] x inv(G[S]) | I_X] and order = S then E (S: the first k
    present shards in index order, E: the rest)."""
    G = rn.build_matrix(k, p, kind)
    Q = [i for i in range(k + p) if present[i]]
    S, E = Q[:k], Q[k:]
    C = rn.matmul(G[E], rn.invert(G[S]))
    return np.concatenate([C, np.eye(len(E), dtype=np.uint8)], axis=1), S + E


def patterns(n, max_missing):
    for m in range(max_missing + 1):
        for lost in itertools.combinations(range(n), m):
            yield [i not in lost for i in range(n)]


@pytest.mark.parametrize("kind", ["vandermonde", "cauchy"])
@pytest.mark.parametrize("k,p,max_missing", [(4, 2, 0), (6, 3, 1), (10, 2, 0), (10, 4, 2)])
def test_check_matrix_matches_numpy(k, p, max_missing, kind):
    """Every pattern with at least k+2 present (RS(4+2), RS(6+3)); RS(10+2)
    and RS(10+4) with 0-2 missing."""
    enc = ia.New(k, p, matrix=kind)
    count = 0
    for present in patterns(k + p, max_missing):
        H, order = enc.check_matrix(present)
        want_H, want_order = ref_check_matrix(k, p, kind, present)
        assert order == want_order, present
        assert H.shape == want_H.shape and np.array_equal(H, want_H), present
        count += 1
    assert count == sum(1 for _ in patterns(k + p, max_missing)) > 0


def test_check_matrix_takes_any_nonzero_flag():
    enc = ia.New(6, 3)
    present = [7, 0, 1, 255, 1, 1, 2, 1, 1]
    H, order = enc.check_matrix(present)
    want_H, want_order = ref_check_matrix(6, 3, "vandermonde", present)
    assert order == want_order and np.array_equal(H, want_H)


def _codes():
    import re
    src = open(_lib.HEADER).read()
    return dict((m[0], int(m[1])) for m in re.findall(r"#define (RSGPU_ERR_\w+) (-?\d+)", src))


def test_error_table_without_device():
    """Each row of the header's table, through every entry point that takes a
    pattern; none of them reaches a device (the pointers are never read)."""
    L = _lib.load()
    E = _codes()
    base, out = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 24)

    def calls(enc, present, S=64, pitch=64, stride=None, base=base):
        n = enc.Shards
        pr = (ctypes.c_uint8 * n)(*[1 if x else 0 for x in present])
        stride = n * pitch if stride is None else stride
        H = (ctypes.c_uint8 * (n * n))()
        order = (ctypes.c_int * n)()
        x = ctypes.c_int()
        loc, ok = ctypes.c_int(), ctypes.c_int()
        bufs = [np.zeros(S, np.uint8) for _ in range(n)]
        ptrs = (ctypes.c_void_p * n)(*[b.ctypes.data for b in bufs])
        lens = (ctypes.c_size_t * n)(*[S if x else 0 for x in present])
        ptrs = ctypes.cast(ptrs, _lib.u8pp)
        return {
            "check_matrix": L.rsgpu_check_matrix(enc._ctx, pr, ctypes.cast(H, _lib.u8p), order, ctypes.byref(x)),
            "locate_dev": L.rsgpu_locate_dev(enc._ctx, base, pr, S, pitch, stride, 2, out, None, None),
            "repair_dev": L.rsgpu_repair_dev(enc._ctx, base, pr, S, pitch, stride, 2, out, out, out, None),
            "locate": L.rsgpu_locate(enc._ctx, ptrs, lens, n, ctypes.byref(loc)),
            "repair": L.rsgpu_repair(enc._ctx, ptrs, lens, n, ctypes.byref(loc), ctypes.byref(ok)),
        }

    def all_are(res, code, names=None):
        for name, got in res.items():
            if names is None or name in names:
                assert got == code, (name, got, code)

    # fewer than k+2 present
    enc = ia.New(10, 2)
    all_are(calls(enc, [0] + [1] * 11), E["RSGPU_ERR_TOO_FEW_SHARDS"])
    all_are(calls(enc, [0] * 3 + [1] * 9), E["RSGPU_ERR_TOO_FEW_SHARDS"])
    enc63 = ia.New(6, 3)
    all_are(calls(enc63, [1] * 7 + [0, 0]), E["RSGPU_ERR_TOO_FEW_SHARDS"])
    # X > 4
    all_are(calls(ia.New(4, 5), [1] * 9), E["RSGPU_ERR_NOT_IMPLEMENTED"])
    all_are(calls(ia.New(10, 6), [1] * 16), E["RSGPU_ERR_NOT_IMPLEMENTED"])
    # more than 16 shards (X within range), after the too-few check
    enc17 = ia.New(14, 3)
    all_are(calls(enc17, [1] * 17), E["RSGPU_ERR_NOT_IMPLEMENTED"])
    all_are(calls(enc17, [0, 0] + [1] * 15), E["RSGPU_ERR_TOO_FEW_SHARDS"])
    # survivors' matrix singular: PAR1 is not MDS (RS(10+6), 12 present: the
    # survivors hold parity rows 0, 1 and 3 against the lost columns 0, 1, 2)
    par1 = ia.New(10, 6, matrix="par1")
    lost = (0, 1, 2, 12)
    singular = [i not in lost for i in range(16)]
    with pytest.raises(rn.Singular):
        rn.invert(rn.build_matrix(10, 6, "par1")[[i for i in range(16) if singular[i]][:10]])
    all_are(calls(par1, singular), E["RSGPU_ERR_SINGULAR"])
    # misaligned or oversized layouts (device calls), after the pattern's checks
    dev = ("locate_dev", "repair_dev")
    all_are(calls(enc, [1] * 12, S=100, pitch=100), E["RSGPU_ERR_INVALID_ARG"], dev)          # pitch % 16
    all_are(calls(enc, [1] * 12, S=100, pitch=112, stride=12 * 112 + 8), E["RSGPU_ERR_INVALID_ARG"], dev)
    all_are(calls(enc, [1] * 12, base=ctypes.c_void_p((1 << 20) + 8)), E["RSGPU_ERR_INVALID_ARG"], dev)
    all_are(calls(enc, [1] * 12, S=100, pitch=96), E["RSGPU_ERR_INVALID_ARG"], dev)           # pitch < S
    all_are(calls(enc, [1] * 12, base=ctypes.c_void_p(0)), E["RSGPU_ERR_INVALID_ARG"], dev)
    big = 400 << 20
    all_are(calls(enc, [1] * 12, S=64, pitch=big), E["RSGPU_ERR_INVALID_ARG"], dev)           # 12 rows >= 4 GiB
    all_are(calls(enc, [0] + [1] * 11, S=100, pitch=100), E["RSGPU_ERR_TOO_FEW_SHARDS"], dev)  # precedence
    # a valid call gets as far as the device
    if not ia.device_ok(0):
        res = calls(enc, [1] * 12)
        all_are(res, E["RSGPU_ERR_NO_DEVICE"], ("locate_dev", "repair_dev", "locate", "repair"))
        assert res["check_matrix"] == 0


def test_python_errors_and_constants():
    assert ia.LOC_CLEAN == -1 and ia.LOC_UNLOCATABLE == -2
    src = open(_lib.HEADER).read()
    assert "#define RSGPU_LOC_CLEAN (-1)" in src and "#define RSGPU_LOC_UNLOCATABLE (-2)" in src
    enc = ia.New(10, 2)
    sh = [np.zeros(8, np.uint8) for _ in range(12)]
    with pytest.raises(ia.ErrTooFewShards):
        enc.Locate([None] + sh[1:])
    with pytest.raises(ia.ErrTooFewShards):
        enc.Repair([None] + sh[1:])
    with pytest.raises(ia.ErrTooFewShards):
        enc.check_matrix([0] + [1] * 11)
    with pytest.raises(ia.ErrTooFewShards):
        enc.Locate(sh[:11])
    with pytest.raises(ia.ErrShardSize):
        enc.Locate(sh[:11] + [np.zeros(7, np.uint8)])
    with pytest.raises(ia.InvalidArgument):
        enc.Repair(tuple(sh))


# ---------------------------------------------------------------- Client.decode


class StubCodec:
    """Verify always fails (a silently corrupted shard); Repair as told."""

    def __init__(self, k, repair_result):
        self.k = k
        self.repair_result = repair_result
        self.repair_calls = []

    def Verify(self, shards):
        return False

    def Reconstruct(self, shards):
        for i, s in enumerate(shards):
            if s is None:
                shards[i] = bytearray(b"?" * 4)

    def Repair(self, shards):
        self.repair_calls.append([None if s is None else bytes(s) for s in shards])
        if self.repair_result[0] >= 0 and self.repair_result[1]:
            for i, s in enumerate(shards):
                shards[i] = bytearray(b"%04d" % i)  # healed and filled
        return self.repair_result

    def Join(self, dst, shards, outSize):
        ia.ec._join(self.k, dst, shards, outSize)


def _client(stub, **kw):
    c = Client(4, 0, 0, **kw)  # p == 0: no GPU codec is created
    c.EC = stub
    return c


def _chunks():
    return [bytearray(b"xxxx"), None, bytearray(b"yyyy"), bytearray(b"zzzz"), bytearray(b"wwww"), bytearray(b"vvvv")]


MESSAGE = "Verification failed after reconstruction, data could be corrupted"


def test_client_decode_repairs():
    stub = StubCodec(4, (3, True))
    c = _client(stub, repair=True)
    stats = DataEntry()
    out = c.decode(stats, _chunks(), 16)
    assert isinstance(out, io.BytesIO) and out.read() == b"0000000100020003"
    assert stats.Repaired == 3 and stats.Corrupted is True and stats.AllGood is False
    # Repair saw the shards as they arrived: the row Reconstruct filled is missing again
    assert stub.repair_calls == [[b"xxxx", None, b"yyyy", b"zzzz", b"wwww", b"vvvv"]]
    c.Close()


@pytest.mark.parametrize("repair,result", [(False, (3, True)), (True, (-2, False)), (True, (-1, True)),
                                            (True, (3, False))])
def test_client_decode_raises_as_before(repair, result):
    stub = StubCodec(4, result)
    c = _client(stub, repair=repair)
    stats = DataEntry()
    with pytest.raises(ia.RSError) as ei:
        c.decode(stats, _chunks(), 16)
    assert str(ei.value) == MESSAGE and type(ei.value) is ia.RSError
    assert stats.Repaired is None and stats.Corrupted is False
    assert len(stub.repair_calls) == (1 if repair else 0)
    c.Close()


def test_client_repair_is_off_by_default():
    c = Client(4, 0, 0)
    assert c.repair is False and DataEntry().Repaired is None
    c.Close()


def test_client_decode_without_repair_method():
    """A codec that has no Repair (DummyEncoder, another implementation)."""
    class NoRepair:
        Verify = staticmethod(lambda shards: False)
        Reconstruct = staticmethod(lambda shards: None)

    c = _client(NoRepair(), repair=True)
    with pytest.raises(ia.RSError) as ei:
        c.decode(DataEntry(), [bytearray(b"xxxx")] * 6, 16)
    assert str(ei.value) == MESSAGE
    c.Close()
