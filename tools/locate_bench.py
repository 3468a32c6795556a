"""Device time of the corrupted-shard locator beside Verify.

RS(10+2), 1 MiB objects, batch 1024, device-resident; three batches coded in
rotation, as bench.py does, so that none is left in the Infinity Cache.  One
process times, with HIP events, several windows each of

    verify_dev          clean batches (the parent's check-only pass, same 12 rows)
    locate_dev          the same clean batches
    locate_dev          batches whose every object has one whole shard randomised
    repair_dev          those batches (re-corrupted, untimed, after every call)

and writes one JSON document (default profiles/locate_bench.json).

    python tools/locate_bench.py [--nobj 1024] [--windows 5] [--steps 6] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nobj", type=int, default=1024)
    ap.add_argument("--obj-bytes", type=int, default=1 << 20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--steps", type=int, default=6, help="calls per window (a multiple of the 3 batches)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "locate_bench.json"))
    args = ap.parse_args()

    import torch

    import infinicache_amd as ia

    if not ia.device_ok(0):
        sys.exit("locate_bench: no usable gfx950 device")
    k, p, copies = 10, 2, 3
    n = k + p
    nobj = args.nobj
    S = (args.obj_bytes + k - 1) // k
    pitch = (S + 255) // 256 * 256
    stride = n * pitch
    dev = "cuda:0"
    enc = ia.New(k, p)
    stream = torch.cuda.current_stream()
    g = torch.Generator(device=dev).manual_seed(0x10CA7E)
    present = [1] * n

    clean = torch.randint(0, 256, (copies, nobj, n, pitch), dtype=torch.uint8, device=dev, generator=g)
    clean[..., S:] = 0
    enc.encode_dev(clean, S, pitch, stride, nobj * copies, stream)
    dirty = clean.clone()
    obj = torch.arange(nobj, device=dev)
    shard = obj % n  # object o: shard o mod 12 randomised whole
    saved = []
    for j in range(copies):
        rows = torch.randint(0, 256, (nobj, pitch), dtype=torch.uint8, device=dev, generator=g)
        rows[:, S:] = 0
        dirty[j, obj, shard] = rows
        saved.append(rows)
    bad = torch.zeros(nobj, dtype=torch.int32, device=dev)
    loc = torch.zeros(nobj, dtype=torch.int32, device=dev)
    masks = torch.zeros(nobj, dtype=torch.int32, device=dev)
    status = torch.zeros(nobj, dtype=torch.int32, device=dev)

    def verify(j):
        enc.verify_dev(clean[j], S, pitch, stride, nobj, bad, stream)

    def locate_clean(j):
        enc.locate_dev(clean[j], present, S, pitch, stride, nobj, loc, masks, stream)

    def locate_dirty(j):
        enc.locate_dev(dirty[j], present, S, pitch, stride, nobj, loc, masks, stream)

    def repair(j):
        enc.repair_dev(dirty[j], present, S, pitch, stride, nobj, loc, masks, status, stream)

    def recorrupt(j):
        dirty[j, obj, shard] = saved[j]

    # results first (and the warm-up of every shape): nothing is timed that is wrong
    checks = {}
    verify(0)
    locate_clean(0)
    torch.cuda.synchronize()
    checks["verify_clean_flags"] = int(bad.sum())
    checks["locate_clean_all_clean"] = bool((loc == ia.LOC_CLEAN).all())
    locate_dirty(1)
    torch.cuda.synchronize()
    checks["locate_dirty_all_named"] = bool((loc == shard.to(torch.int32)).all())
    repair(1)
    torch.cuda.synchronize()
    checks["repair_all_healed"] = bool((status == 0).all()) and bool(torch.equal(dirty[1], clean[1]))
    recorrupt(1)
    torch.cuda.synchronize()
    if not (checks["verify_clean_flags"] == 0 and checks["locate_clean_all_clean"] and
            checks["locate_dirty_all_named"] and checks["repair_all_healed"]):
        sys.exit("locate_bench: wrong results, nothing timed: %r" % checks)

    def windows(fn, after=None):
        """ms per call of each window; every call between its own pair of events
        (so the untimed `after` step, on the same stream, stays outside)."""
        out = []
        step = 0
        for _ in range(args.warmup):
            fn(step % copies)
            if after:
                after(step % copies)
            step += 1
        for _ in range(args.windows):
            ev = []
            for _ in range(args.steps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                fn(step % copies)
                e1.record(stream)
                if after:
                    after(step % copies)
                ev.append((e0, e1))
                step += 1
            torch.cuda.synchronize()
            out.append(sum(a.elapsed_time(b) for a, b in ev) / args.steps)
        return out

    read_bytes = nobj * n * S  # the 12 rows every pass reads
    res = {}
    # verify and clean locate alternate window by window in the same process
    runs = [("verify_clean", verify, None), ("locate_clean", locate_clean, None),
            ("locate_one_shard_randomised", locate_dirty, None), ("repair_one_shard_randomised", repair, recorrupt)]
    for name, fn, after in runs:
        ms = windows(fn, after)
        res[name] = {
            "ms_per_call_windows": [round(x, 4) for x in ms],
            "ms_per_call_median": round(statistics.median(ms), 4),
            "spread_pct": round(100.0 * (max(ms) - min(ms)) / statistics.median(ms), 2),
            "read_GBps_median": round(read_bytes / statistics.median(ms) / 1e6, 1),
        }
    doc = {
        "tool": "tools/locate_bench.py",
        "code": "RS(10+2) vandermonde", "obj_bytes": args.obj_bytes, "shard_len": S, "pitch": pitch, "nobj": nobj,
        "batches_in_rotation": copies, "batch_bytes": nobj * stride,
        "windows": args.windows, "calls_per_window": args.steps, "warmup_calls": args.warmup,
        "timing": "HIP events around every call on the call's stream; ms per call, mean of each window",
        "read_bytes_per_call": read_bytes,
        "device": torch.cuda.get_device_name(0),
        "checks": checks,
        "results": res,
        "locate_clean_over_verify": round(res["locate_clean"]["ms_per_call_median"] /
                                          res["verify_clean"]["ms_per_call_median"], 4),
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
