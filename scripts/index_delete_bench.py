"""Dedup index, delete path: the time of fdfs_gpu_index_lookup, _remove and
_ingest for one batch against an index that holds --classes classes
(DESIGN.md 4.8).  The batch is --batch records drawn uniformly from the
classes the index holds (so it repeats some of them); each round looks the
batch up, ingests it (every class a hit: ref += members) and removes it (ref
back to what it was, no class reaches 0), so every round meets the same
index (the first ingest may grow the table: the host makes room for a batch
of all-new classes; that falls into the warm-up).  Two clocks per call, median of --reps rounds after --warmup:
  pair_ms: the library's FDFS_KERNEL_DEDUP event pair (fdfs_gpu_set_timing /
           fdfs_gpu_read_timing).  For lookup and remove it spans the whole
           call; for ingest it spans the batch's grouping only, as it always
           has (the upsert and answer kernels are outside it).
  call_ms: device events around the whole call, the like-for-like figure.
A last pair of calls removes the whole batch from a fresh copy of the state
(every class of it reaches 0: tombstones) and looks it up again (all misses).

usage: python3 scripts/index_delete_bench.py [--classes N] [--batch N] [--reps N] [--warmup N]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import fastdfs_amd as F  # noqa: E402
from fastdfs_amd import _lib  # noqa: E402
from fastdfs_amd.api import DedupIndex  # noqa: E402


def sigs_of(cls):
    """Distinct 24-byte signatures of int64 class ids (device)."""
    words = torch.stack([cls, cls * 0x9E3779B97F4A7C15 + 12345, cls ^ 0x5555AAAA5555AAAA], dim=1)
    return words.contiguous().view(torch.uint8).view(cls.numel(), 24)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--classes", type=int, default=50_000_000)
    ap.add_argument("--batch", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    ctx = F.Context(0)
    ix = DedupIndex(ctx, a.classes)
    for lo in range(0, a.classes, a.batch):  # build: every class once
        hi = min(a.classes, lo + a.batch)
        ix.ingest(sigs_of(torch.arange(lo, hi, dtype=torch.int64, device=dev)))
    torch.cuda.synchronize()
    built = ix.stats()
    assert built["classes"] == a.classes and built["unplaced"] == 0, built
    g = torch.Generator(device=dev)
    g.manual_seed(50)
    ids = torch.randint(0, a.classes, (a.batch,), generator=g, device=dev, dtype=torch.int64)
    batch = sigs_of(ids)
    distinct = int(torch.unique(ids).numel())
    del ids
    ctx.set_timing(True)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(fn):
        torch.cuda.synchronize()
        ctx.read_timing(_lib.KERNEL_DEDUP)
        ev[0].record()
        out = fn(batch)
        ev[1].record()
        torch.cuda.synchronize()
        pair, launches = ctx.read_timing(_lib.KERNEL_DEDUP)
        assert launches == 1
        return out, pair, ev[0].elapsed_time(ev[1])

    t = {k: {"pair_ms": [], "call_ms": []} for k in ("lookup", "ingest", "remove")}
    for r in range(a.warmup + a.reps):
        for name, fn in (("lookup", ix.lookup), ("ingest", ix.ingest), ("remove", ix.remove)):
            out, pair, call = timed(fn)
            if r >= a.warmup:
                t[name]["pair_ms"].append(pair)
                t[name]["call_ms"].append(call)
            if name == "remove":
                assert int(out[1].min()) == 1  # ref back to 1: the round left the index as it found it
        assert ix.stats()["classes"] == a.classes
    res = {"device": torch.cuda.get_device_name(0), "classes": a.classes, "batch": a.batch,
           "batch_distinct": distinct, "slots_built": built["slots"], "slots": ix.stats()["slots"],
           "reps": a.reps, "warmup": a.warmup}
    for k, v in t.items():
        for c, x in v.items():
            res[f"{k}_{c}"] = round(float(np.median(x)), 3)
            res[f"{k}_{c}_minmax"] = [round(float(min(x)), 3), round(float(max(x)), 3)]
    # once: the batch's classes all reach 0, then are looked up as misses
    out, pair, call = timed(ix.remove)
    res["remove_to_zero_call_ms"] = round(call, 3)
    st = ix.stats()
    assert int(out[1].max()) == 0 and st["tombstones"] == distinct and st["classes"] == a.classes - distinct, st
    out, pair, call = timed(ix.lookup)
    res["lookup_miss_call_ms"] = round(call, 3)
    assert int(out[0].max()) == -1
    print(json.dumps(res), flush=True)
    ix.close()
    ctx.close()


if __name__ == "__main__":
    main()
