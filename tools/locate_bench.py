"""Device time of the corrupted-shard locator beside Verify.

RS(10+2), 1 MiB objects, batch 1024, device-resident; three batches coded in
rotation, as bench.py does, so that none is left in the Infinity Cache.  One
process times, with HIP events, several windows each of

    verify_dev          clean batches (the parent's check-only pass, same 12 rows)
    locate_dev          the same clean batches
    locate_dev          batches whose every object has one whole shard randomised
    repair_dev          those batches (re-corrupted, untimed, after every call)

and writes one JSON document (default profiles/locate_bench.json).

The per-object calls (rsgpu_locate_dev_masks) are timed in the same process
and windows, and go into a second document (default
profiles/locate_masks_bench.json):

    (a) locate_dev_masks, every mask 0xFFF, on the clean and dirty batches
        above, beside locate_dev on the same batches;
    (b) RS(10+4), 1 MiB objects, the Get mix (object o: all present, shard 3
        lost, shards {0,5} lost, by o mod 3): one locate_dev_masks call
        against the three per-pattern locate_dev calls over the same objects
        (each a strided third of the batch), clean and dirty; and once more
        in a fresh process with RSGPU_LOCATE_XPAD=1 (the long-row kernel's
        largest-X body for every object instead of a branch on X);
    (c) RS(10+2), 4 KiB objects (S = 410), batch 65,536: the short-row form
        against the long-row form, the latter in a fresh process with
        RSGPU_LOCATE_LANES=0 (the switch is read at load).

    python tools/locate_bench.py [--nobj 1024] [--windows 5] [--steps 6] [--out FILE] [--masks-out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
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
    ap.add_argument("--masks-out", default=os.path.join(ROOT, "profiles", "locate_masks_bench.json"))
    ap.add_argument("--small-nobj", type=int, default=65536)
    ap.add_argument("--child", choices=("mix", "small"), help="(internal) one masks line in this process, JSON on stdout")
    args = ap.parse_args()

    import torch

    import infinicache_amd as ia

    if not ia.device_ok(0):
        sys.exit("locate_bench: no usable gfx950 device")
    if args.child:
        line = (bench_mix if args.child == "mix" else bench_small)(args, torch, ia)
        print("CHILD " + json.dumps(line))
        return
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

    full = torch.full((nobj,), (1 << n) - 1, dtype=torch.int32, device=dev)
    loc_m = torch.zeros(nobj, dtype=torch.int32, device=dev)
    masks_m = torch.zeros(nobj, dtype=torch.int32, device=dev)

    def locate_masks_clean(j):
        enc.locate_dev_masks(clean[j], full, S, pitch, stride, nobj, loc_m, masks_m, stream)

    def locate_masks_dirty(j):
        enc.locate_dev_masks(dirty[j], full, S, pitch, stride, nobj, loc_m, masks_m, stream)

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
    locate_masks_clean(0)
    torch.cuda.synchronize()
    checks["locate_masks_clean_all_clean"] = bool((loc_m == ia.LOC_CLEAN).all()) and bool((masks_m == full).all())
    locate_masks_dirty(1)
    torch.cuda.synchronize()
    checks["locate_masks_dirty_all_named"] = bool((loc_m == shard.to(torch.int32)).all())
    if not (checks["verify_clean_flags"] == 0 and checks["locate_clean_all_clean"] and
            checks["locate_dirty_all_named"] and checks["repair_all_healed"] and
            checks["locate_masks_clean_all_clean"] and checks["locate_masks_dirty_all_named"]):
        sys.exit("locate_bench: wrong results, nothing timed: %r" % checks)

    def windows(fn, after=None):
        return timed_windows(args, torch, stream, copies, fn, after)

    read_bytes = nobj * n * S  # the 12 rows every pass reads
    res = {}
    # verify and clean locate alternate window by window in the same process
    runs = [("verify_clean", verify, None), ("locate_clean", locate_clean, None),
            ("locate_masks_clean", locate_masks_clean, None),
            ("locate_one_shard_randomised", locate_dirty, None),
            ("locate_masks_one_shard_randomised", locate_masks_dirty, None),
            ("repair_one_shard_randomised", repair, recorrupt)]
    for name, fn, after in runs:
        res[name] = summary(windows(fn, after), read_bytes)
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
    masks_res = {k_: res.pop(k_) for k_ in ("locate_masks_clean", "locate_masks_one_shard_randomised")}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))

    # ---- the per-object calls' own document
    del clean, dirty, saved
    torch.cuda.empty_cache()
    line_a = {
        "what": "RS(10+2), every mask 0xFFF, same batches, process and windows as locate_dev above",
        "locate_dev_clean": res["locate_clean"], "locate_dev_masks_clean": masks_res["locate_masks_clean"],
        "locate_dev_dirty": res["locate_one_shard_randomised"],
        "locate_dev_masks_dirty": masks_res["locate_masks_one_shard_randomised"],
        "masks_over_uniform_clean": round(masks_res["locate_masks_clean"]["ms_per_call_median"] /
                                          res["locate_clean"]["ms_per_call_median"], 4),
        "masks_over_uniform_dirty": round(masks_res["locate_masks_one_shard_randomised"]["ms_per_call_median"] /
                                          res["locate_one_shard_randomised"]["ms_per_call_median"], 4),
    }
    line_b = bench_mix(args, torch, ia)
    torch.cuda.empty_cache()
    line_b["xpad_process"] = child(args, "mix", {"RSGPU_LOCATE_XPAD": "1"})
    line_c = bench_small(args, torch, ia)
    torch.cuda.empty_cache()
    line_c["long_row_form_process"] = child(args, "small", {"RSGPU_LOCATE_LANES": "0"})
    line_c["long_over_short"] = round(line_c["long_row_form_process"]["locate_dev_masks_clean"]["ms_per_call_median"] /
                                      line_c["locate_dev_masks_clean"]["ms_per_call_median"], 3)
    mdoc = {
        "tool": "tools/locate_bench.py",
        "windows": args.windows, "calls_per_window": args.steps, "warmup_calls": args.warmup,
        "batches_in_rotation": copies,
        "timing": "HIP events around every call on the call's stream; ms per call, mean of each window",
        "device": torch.cuda.get_device_name(0),
        "checks": checks,
        "a_uniform_mask": line_a, "b_get_mix": line_b, "c_small_objects": line_c,
    }
    with open(args.masks_out, "w") as f:
        json.dump(mdoc, f, indent=1)
        f.write("\n")
    print(json.dumps(mdoc))


def timed_windows(args, torch, stream, copies, fn, after=None):
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


def summary(ms, read_bytes):
    return {
        "ms_per_call_windows": [round(x, 4) for x in ms],
        "ms_per_call_median": round(statistics.median(ms), 4),
        "spread_pct": round(100.0 * (max(ms) - min(ms)) / statistics.median(ms), 2),
        "read_GBps_median": round(read_bytes / statistics.median(ms) / 1e6, 1),
    }


def child(args, which, env):
    """One masks line in a fresh process (the switches are read at load)."""
    cmd = [sys.executable, os.path.abspath(__file__), "--child", which, "--nobj", str(args.nobj),
           "--obj-bytes", str(args.obj_bytes), "--windows", str(args.windows), "--steps", str(args.steps),
           "--warmup", str(args.warmup), "--small-nobj", str(args.small_nobj)]
    r = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, **env), timeout=600)
    for ln in r.stdout.splitlines():
        if ln.startswith("CHILD "):
            out = json.loads(ln[6:])
            out["env"] = env
            return out
    sys.exit("locate_bench: child %s failed: %s" % (which, (r.stdout + r.stderr)[-2000:]))


def bench_mix(args, torch, ia):
    """(b): RS(10+4), the Get mix, one masked call against three uniform ones."""
    k, p, copies = 10, 4, 3
    n = k + p
    nobj = args.nobj // 3 * 3
    S = (args.obj_bytes + k - 1) // k
    pitch = (S + 255) // 256 * 256
    stride = n * pitch
    dev = "cuda:0"
    enc = ia.New(k, p)
    stream = torch.cuda.current_stream()
    g = torch.Generator(device=dev).manual_seed(0x6E7)
    patterns = [(), (3,), (0, 5)]  # object o: patterns[o % 3]
    pres = [[0 if i in lost else 1 for i in range(n)] for lost in patterns]
    pmask = [sum(1 << i for i in range(n) if pr[i]) for pr in pres]
    obj = torch.arange(nobj, device=dev)
    present = torch.tensor(pmask, dtype=torch.int32, device=dev)[obj % 3].contiguous()
    clean = torch.randint(0, 256, (copies, nobj, n, pitch), dtype=torch.uint8, device=dev, generator=g)
    clean[..., S:] = 0
    enc.encode_dev(clean, S, pitch, stride, nobj * copies, stream)
    dirty = clean.clone()
    shard = 7 + obj % 7  # shards 7..13 are present in all three patterns
    for j in range(copies):
        rows = torch.randint(0, 256, (nobj, pitch), dtype=torch.uint8, device=dev, generator=g)
        rows[:, S:] = 0
        dirty[j, obj, shard] = rows
    loc = torch.zeros(nobj, dtype=torch.int32, device=dev)
    masks = torch.zeros(nobj, dtype=torch.int32, device=dev)
    loc_u = torch.zeros(nobj, dtype=torch.int32, device=dev)
    masks_u = torch.zeros(nobj, dtype=torch.int32, device=dev)

    def masked(buf):
        return lambda j: enc.locate_dev_masks(buf[j], present, S, pitch, stride, nobj, loc, masks, stream)

    def per_pattern(buf):
        def run(j):
            for t in range(3):  # the objects of pattern t: a strided third of the batch
                enc.locate_dev(buf[j, t:], pres[t], S, pitch, 3 * stride, nobj // 3, loc_u[t * (nobj // 3):],
                               masks_u[t * (nobj // 3):], stream)
        return run

    def grouped(x):  # masked results in the per-pattern calls' order
        return torch.cat([x[t::3] for t in range(3)])

    checks = {}
    masked(clean)(0)
    per_pattern(clean)(0)
    torch.cuda.synchronize()
    checks["clean_all_clean"] = bool((loc == ia.LOC_CLEAN).all()) and bool(torch.equal(grouped(loc), loc_u))
    masked(dirty)(1)
    per_pattern(dirty)(1)
    torch.cuda.synchronize()
    checks["dirty_all_named"] = bool((loc == shard.to(torch.int32)).all())
    checks["equals_per_pattern_calls"] = bool(torch.equal(grouped(loc), loc_u)) and bool(torch.equal(grouped(masks), masks_u))
    if not all(checks.values()):
        sys.exit("locate_bench (mix): wrong results, nothing timed: %r" % checks)
    read_bytes = sum(nobj // 3 * (n - len(lost)) * S for lost in patterns)
    line = {"what": "RS(10+4), 1 MiB objects, masks by o mod 3: all present / shard 3 lost / shards {0,5} lost",
            "nobj": nobj, "shard_len": S, "pitch": pitch, "read_bytes_per_call": read_bytes, "checks": checks}
    for name, fn in (("per_pattern_locate_dev_x3_clean", per_pattern(clean)), ("locate_dev_masks_clean", masked(clean)),
                     ("per_pattern_locate_dev_x3_dirty", per_pattern(dirty)), ("locate_dev_masks_dirty", masked(dirty))):
        line[name] = summary(timed_windows(args, torch, stream, copies, fn), read_bytes)
    for st in ("clean", "dirty"):
        line["masks_over_per_pattern_" + st] = round(line["locate_dev_masks_" + st]["ms_per_call_median"] /
                                                     line["per_pattern_locate_dev_x3_" + st]["ms_per_call_median"], 4)
    return line


def bench_small(args, torch, ia):
    """(c): RS(10+2), 4 KiB objects, whichever form this process's switch selects."""
    k, p, copies = 10, 2, 3
    n = k + p
    nobj = args.small_nobj
    S = (4096 + k - 1) // k
    pitch = (S + 15) // 16 * 16
    stride = n * pitch
    dev = "cuda:0"
    enc = ia.New(k, p)
    stream = torch.cuda.current_stream()
    g = torch.Generator(device=dev).manual_seed(0x4C)
    clean = torch.randint(0, 256, (copies, nobj, n, pitch), dtype=torch.uint8, device=dev, generator=g)
    clean[..., S:] = 0
    enc.encode_dev(clean, S, pitch, stride, nobj * copies, stream)
    dirty = clean.clone()
    obj = torch.arange(nobj, device=dev)
    shard = obj % n
    for j in range(copies):
        rows = torch.randint(0, 256, (nobj, pitch), dtype=torch.uint8, device=dev, generator=g)
        rows[:, S:] = 0
        dirty[j, obj, shard] = rows
    present = torch.full((nobj,), (1 << n) - 1, dtype=torch.int32, device=dev)
    loc = torch.zeros(nobj, dtype=torch.int32, device=dev)
    masks = torch.zeros(nobj, dtype=torch.int32, device=dev)

    def masked(buf):
        return lambda j: enc.locate_dev_masks(buf[j], present, S, pitch, stride, nobj, loc, masks, stream)

    checks = {}
    masked(clean)(0)
    torch.cuda.synchronize()
    checks["clean_all_clean"] = bool((loc == ia.LOC_CLEAN).all())
    masked(dirty)(1)
    torch.cuda.synchronize()
    checks["dirty_all_named"] = bool((loc == shard.to(torch.int32)).all())
    if not all(checks.values()):
        sys.exit("locate_bench (small): wrong results, nothing timed: %r" % checks)
    read_bytes = nobj * n * S
    line = {"what": "RS(10+2), 4 KiB objects, every mask 0xFFF", "nobj": nobj, "shard_len": S, "pitch": pitch,
            "read_bytes_per_call": read_bytes, "checks": checks,
            "form": "long rows (RSGPU_LOCATE_LANES=0)" if os.environ.get("RSGPU_LOCATE_LANES") == "0" else "short rows"}
    for name, fn in (("locate_dev_masks_clean", masked(clean)), ("locate_dev_masks_dirty", masked(dirty))):
        line[name] = summary(timed_windows(args, torch, stream, copies, fn), read_bytes)
    return line


if __name__ == "__main__":
    main()
