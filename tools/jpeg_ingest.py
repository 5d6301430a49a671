#!/usr/bin/env python3
"""JPEG ingest rate: the per-image rtdm.jpeg.decode loop against rtdm.jpeg.BatchDecoder on
the same files in one process.

  python tools/jpeg_ingest.py [--batch 60] [--tag NAME] [--out FILE]

The 15 bundled JPEGs (tests/golden/jpeg), replicated to the batch size.  Per path: 3 warm-up
calls, then 5 timed calls (host clock, torch.cuda.synchronize() at both ends), the three
paths taking turns inside every round; the median gives frames/s and megapixels/s, the five
times are kept so that the spread can be read.  The batched path's stages are timed in calls
of their own (profile = True): host Huffman ms (wall clock of the threaded stage), copy ms and
device ms (hipEvents around the copy and around the two launches), medians of 5.  Prints
one JSON line (and appends it to --out)."""
import argparse
import glob
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "real-time-disaster-management_amd"))

from rtdm import jpeg as J  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=60)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--tag", default="")
ap.add_argument("--out", default="")
args = ap.parse_args()

files = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "jpeg", "*.jpg")))
assert files, "no fixtures under tests/golden/jpeg"
assert torch.cuda.is_available(), "jpeg_ingest.py measures on the HIP device"
dev = torch.device("cuda", torch.cuda.current_device())
datas = [open(f, "rb").read() for f in files]
datas = [datas[i % len(datas)] for i in range(args.batch)]
pixels = sum(J.info(d).width * J.info(d).height for d in datas)

decoders = {1: J.BatchDecoder(dev, threads=1), 16: J.BatchDecoder(dev, threads=16)}
paths = {"loop": lambda: [J.decode(d, dev) for d in datas],
         "batch_t1": lambda: decoders[1].decode(datas),
         "batch_t16": lambda: decoders[16].decode(datas)}

# the three paths agree bit for bit before anything is timed
ref = paths["loop"]()
for name in ("batch_t1", "batch_t16"):
    got = paths[name]()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(ref, got)), name
del ref, got

times = {name: [] for name in paths}
for rnd in range(args.warmup + args.rounds):
    for name, fn in paths.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        del out
        if rnd >= args.warmup:
            times[name].append(dt * 1e3)

res = {"tool": "jpeg_ingest", "tag": args.tag, "device": torch.cuda.get_device_name(dev), "images": len(datas),
       "distinct_files": len(files), "megapixels": round(pixels / 1e6, 3), "warmup": args.warmup, "rounds": args.rounds}
for name, ts in times.items():
    med = statistics.median(ts)
    res[name] = {"ms_median": round(med, 3), "ms_all": [round(t, 3) for t in ts],
                 "frames_per_s": round(len(datas) / med * 1e3, 1), "megapixels_per_s": round(pixels / med / 1e3, 1)}
for thr, dec in decoders.items():
    dec.profile = True
    stages = []
    for rnd in range(args.warmup + args.rounds):
        torch.cuda.synchronize()
        out = dec.decode(datas)
        t = dec.timings()
        torch.cuda.synchronize()
        del out
        if rnd >= args.warmup:
            stages.append(t)
    dec.profile = False
    res[f"batch_t{thr}"]["stages_ms"] = {k: round(statistics.median(s[k] for s in stages), 3) for k in stages[0]}
res["batch_t16_outside_loop_spread"] = res["batch_t16"]["ms_median"] < min(times["loop"])
line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")
