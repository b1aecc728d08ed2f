"""GPU: the delete path of the dedup index (fdfs_gpu_index_remove,
fdfs_gpu_index_lookup, tombstones, compaction) against a model.

The model is the FastDHT state itself as a dict, signature bytes -> [source
gidx, ref], with every operation applied batch-wise as include/fdfs_gpu.h
states it: an ingest answers after the whole batch (source = first file ever
with the signature since its class last vanished), a remove takes min(ref,
members in the batch) off and drops the class at 0, a lookup reads."""
import ctypes
import errno

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NONE = -1  # api.INDEX_NONE


@pytest.fixture(scope="module")
def ctx():
    import fastdfs_amd as F
    if not torch.cuda.is_available():
        pytest.fail("gpu test collected without a GPU")
    return F.Context(0)


def _sigs(n, nuniq, seed):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, size=(nuniq, 24), dtype=np.uint8)
    return base[rng.integers(0, nuniq, size=n)]


def _distinct(n, seed):
    s = np.random.default_rng(seed).integers(0, 256, size=(n, 24), dtype=np.uint8)
    assert np.unique(s, axis=0).shape[0] == n
    return s


class Model:
    def __init__(self):
        self.d = {}
        self.records = 0

    def ingest(self, sig, gidx=None):
        keys = [r.tobytes() for r in sig]
        for i, k in enumerate(keys):
            e = self.d.setdefault(k, [int(gidx[i]) if gidx is not None else self.records + i, 0])
            e[1] += 1
        self.records += len(keys)
        return (np.array([self.d[k][0] for k in keys], np.int64).reshape(-1),
                np.array([self.d[k][1] for k in keys], np.int32).reshape(-1))

    def lookup(self, sig):
        keys = [r.tobytes() for r in sig]
        return (np.array([self.d[k][0] if k in self.d else NONE for k in keys], np.int64).reshape(-1),
                np.array([self.d[k][1] if k in self.d else 0 for k in keys], np.int32).reshape(-1))

    def remove(self, sig):
        """-> rep, ref, unlink, and what the batch exercised."""
        keys = [r.tobytes() for r in sig]
        cnt, first = {}, {}
        for i, k in enumerate(keys):
            cnt[k] = cnt.get(k, 0) + 1
            first.setdefault(k, i)
        ans, unlink = {}, np.zeros(len(keys), np.uint8)
        seen = {"repeat": any(c > 1 for c in cnt.values()), "absent": False, "clamp": False, "partial": False}
        for k, c in cnt.items():
            if k not in self.d:
                ans[k] = (NONE, 0)
                seen["absent"] = True
                continue
            src, ref = self.d[k]
            seen["clamp"] |= c > ref
            left = ref - min(ref, c)
            ans[k] = (src, left)
            if left == 0:
                del self.d[k]
                unlink[first[k]] = 1
            else:
                self.d[k][1] = left
                seen["partial"] = True
        return (np.array([ans[k][0] for k in keys], np.int64).reshape(-1),
                np.array([ans[k][1] for k in keys], np.int32).reshape(-1), unlink, seen)


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


def _ingest(ix, model, sig, gidx=None):
    rep, ref = ix.ingest(_dev(sig), None if gidx is None else _dev(gidx))
    mrep, mref = model.ingest(sig, gidx)
    assert np.array_equal(rep.cpu().numpy(), mrep)
    assert np.array_equal(ref.cpu().numpy(), mref)
    return mrep, mref


def _remove(ix, model, sig):
    rep, ref, unlink = ix.remove(_dev(sig).reshape(-1, 24), want_unlink=True)
    mrep, mref, munlink, seen = model.remove(sig)
    assert np.array_equal(rep.cpu().numpy(), mrep)
    assert np.array_equal(ref.cpu().numpy(), mref)
    assert np.array_equal(unlink.cpu().numpy(), munlink)
    return seen


def _lookup(ix, model, sig):
    rep, ref = ix.lookup(_dev(sig))
    mrep, mref = model.lookup(sig)
    assert np.array_equal(rep.cpu().numpy(), mrep)
    assert np.array_equal(ref.cpu().numpy(), mref)
    return mrep, mref


def _check_stats(ix, model):
    st = ix.stats()
    assert st["classes"] == len(model.d)
    assert st["records"] == model.records
    assert st["unplaced"] == 0
    assert st["classes"] + st["tombstones"] <= st["slots"] * 3 // 4
    return st


def test_lookup_reads_and_changes_nothing(oracle, ctx):
    from fastdfs_amd.api import DedupIndex
    sig = _sigs(5000, 3000, 71)
    absent = _distinct(700, 72)
    ix, model = DedupIndex(ctx, 10_000), Model()
    try:
        mrep, mref = _ingest(ix, model, sig)
        orep, oref = oracle.dedup(sig)  # the model itself against the oracle's sequential dedup
        assert np.array_equal(mrep, orep.astype(np.int64)) and np.array_equal(mref, oref.astype(np.int32))
        rng = np.random.default_rng(73)
        q = np.concatenate([sig[rng.integers(0, 5000, 2500)], absent, sig[:300], absent[:50], sig[:300]])
        q = q[rng.permutation(len(q))]
        before = ix.stats()
        rep1, ref1 = _lookup(ix, model, q)
        assert int((rep1 == NONE).sum()) == 750 and int((ref1[rep1 == NONE] != 0).sum()) == 0
        assert ix.stats() == before
        rep2, ref2 = _lookup(ix, model, q)
        assert np.array_equal(rep1, rep2) and np.array_equal(ref1, ref2)
        assert ix.stats() == before and before["tombstones"] == 0
    finally:
        ix.close()


def test_random_interleaving_matches_model(ctx):
    """About 30 operations, the first ones written out so that every case
    the header names occurs (asserted at the end), the rest drawn."""
    from fastdfs_amd.api import DedupIndex
    rng = np.random.default_rng(20261)
    pool = _distinct(2000, 81)
    never = _distinct(300, 82)  # never ingested
    ix, model = DedupIndex(ctx, 1000), Model()  # small: make_room runs along the way
    seen = {"repeat": False, "absent": False, "clamp": False, "partial": False}
    g = [0]

    def gidx(n):  # explicit, increasing across the stream
        v = g[0] + np.cumsum(rng.integers(1, 5, n)).astype(np.int64)
        g[0] = int(v[-1])
        return v

    def ingest(sig):
        r = _ingest(ix, model, sig, gidx(len(sig)))
        _check_stats(ix, model)
        return r

    def remove(sig):
        s = _remove(ix, model, sig)
        for k in seen:
            seen[k] |= s[k]
        _check_stats(ix, model)
        return s

    try:
        ingest(pool[rng.integers(0, 1500, 3000)])
        _lookup(ix, model, np.concatenate([pool[:900], never[:40], pool[:30]]))
        st0 = _check_stats(ix, model)
        remove(np.zeros((0, 24), np.uint8))  # n = 0: returns, changes nothing
        assert ix.stats() == st0
        one = next(k for k, v in model.d.items() if v[1] >= 2)
        assert remove(np.frombuffer(one, np.uint8).reshape(1, 24))["partial"]  # a single record; part of a class
        # more removes than the class has members, among other records
        ck, (csrc, cref) = next((k, v) for k, v in model.d.items() if v[1] >= 2)
        batch = np.concatenate([pool[1000:1100], np.tile(np.frombuffer(ck, np.uint8), (cref + 3, 1)), never[:20]])
        s = remove(batch[rng.permutation(len(batch))])
        assert s["clamp"] and s["absent"] and s["repeat"] and ck not in model.d
        remove(never[100:160])  # nothing of it was ever ingested
        # the removed class again: a new source, ref counted from 0
        again = np.tile(np.frombuffer(ck, np.uint8), (2, 1))
        gv = gidx(2)
        rep, ref = _ingest(ix, model, again, gv)
        assert rep[0] == rep[1] == gv[0] > csrc and list(ref) == [2, 2]
        _check_stats(ix, model)
        for _ in range(22):
            kind = rng.choice(["ingest", "remove", "lookup"], p=[0.35, 0.4, 0.25])
            n = int(rng.integers(1, 4001))
            sig = pool[rng.integers(0, 2000, n)]
            if kind == "ingest":
                ingest(sig)
            elif kind == "remove":
                k = int(rng.integers(0, 30))
                sig = np.concatenate([sig, never[rng.integers(0, 300, k)]])
                remove(sig[rng.permutation(len(sig))])
            else:
                _lookup(ix, model, np.concatenate([sig, never[:25]]))
                _check_stats(ix, model)
        assert all(seen.values()), seen
        _lookup(ix, model, np.concatenate([pool, never]))
    finally:
        ix.close()


M64 = (1 << 64) - 1
IX_K = 0x632BE59BD9B4E019


def ix_mix(k):
    k ^= k >> 33
    k = k * 0xff51afd7ed558ccd & M64
    k ^= k >> 33
    k = k * 0xc4ceb9fe1a85ec53 & M64
    k ^= k >> 33
    return k


def ix_hash(a, b, c):
    return ix_mix(c ^ ix_mix(b ^ ix_mix((a + IX_K) & M64)))


def test_tombstones_inside_one_probe_chain(ctx):
    """64 signatures with one ix_hash: one probe chain.  Every second one
    removed leaves tombstones between the survivors: a dead slot taken for
    the chain's end would lose the survivors behind it (or insert them
    twice), a reused one could shadow a key further along."""
    from fastdfs_amd.api import DedupIndex
    c, t = 0x0123456789ABCDEF, 0x0F1E2D3C4B5A6978
    rng = np.random.default_rng(91)
    words = []
    for a in (int(x) for x in rng.integers(0, 1 << 63, 64, dtype=np.uint64)):
        words.append((a, t ^ ix_mix((a + IX_K) & M64), c))
    assert len(set(words)) == 64 and len({ix_hash(*w) for w in words}) == 1
    sig = np.array(words, dtype="<u8").view(np.uint8).reshape(64, 24)
    ix, model = DedupIndex(ctx, 1000), Model()
    try:
        _ingest(ix, model, sig, np.arange(100, 164, dtype=np.int64))
        gone, kept = sig[0::2], sig[1::2]
        assert not any(_remove(ix, model, gone).values())  # 32 whole classes, nothing else
        rep, ref = _lookup(ix, model, sig)
        assert list(rep[0::2]) == [NONE] * 32 and list(ref[0::2]) == [0] * 32
        assert list(rep[1::2]) == list(range(101, 164, 2)) and list(ref[1::2]) == [1] * 32
        rep, ref = _ingest(ix, model, kept, np.arange(1000, 1032, dtype=np.int64))
        assert list(rep) == list(range(101, 164, 2)) and list(ref) == [2] * 32
        rep, ref = _ingest(ix, model, gone, np.arange(2000, 2032, dtype=np.int64))
        assert list(rep) == list(range(2000, 2032)) and list(ref) == [1] * 32
        st = _check_stats(ix, model)
        assert st["classes"] == 64 and st["tombstones"] == 32  # no rehash was due: none reclaimed
        _lookup(ix, model, sig)
    finally:
        ix.close()


def test_churn_compacts_instead_of_growing(ctx):
    from fastdfs_amd.api import DedupIndex
    ix, model = DedupIndex(ctx, 10), Model()
    try:
        assert ix.stats()["slots"] == 1024
        for r in range(20):
            sig = _distinct(500, 1000 + r)
            _ingest(ix, model, sig)
            seen = _remove(ix, model, sig)
            assert not any(seen.values())
            assert len(model.d) == 0
        st = _check_stats(ix, model)
        # live classes never exceed 500 < 768: tombstones are dropped, the table never grows
        assert st["slots"] == 1024 and st["classes"] == 0 and st["tombstones"] <= 768
        assert st["records"] == 20 * 500
    finally:
        ix.close()


def test_growth_after_removes_drops_tombstones(ctx):
    from fastdfs_amd.api import DedupIndex
    ix, model = DedupIndex(ctx, 10), Model()
    try:
        first, new = _distinct(600, 2001), _distinct(2000, 2002)
        _ingest(ix, model, first)
        _remove(ix, model, first[:300])
        assert ix.stats()["tombstones"] == 300 and ix.stats()["slots"] == 1024
        _ingest(ix, model, new)
        rep, ref = _lookup(ix, model, first[:300])
        assert (rep == NONE).all() and (ref == 0).all()
        rep, ref = _lookup(ix, model, np.concatenate([first[300:], new]))
        assert (rep != NONE).all() and (ref == 1).all()
        st = _check_stats(ix, model)
        assert st["slots"] >= 4096 and st["tombstones"] == 0 and st["classes"] == 2300
    finally:
        ix.close()


def test_argument_errors(ctx):
    from fastdfs_amd.api import DedupIndex
    L = ctx._L
    ix = DedupIndex(ctx, 100)
    try:
        sig = _dev(_distinct(17, 3001).reshape(-1))[:16 * 24 + 8]
        rep = torch.empty(16, dtype=torch.int64, device="cuda")
        ref = torch.empty(16, dtype=torch.int32, device="cuda")
        p, r, f = sig.data_ptr(), rep.data_ptr(), ref.data_ptr()
        assert L.fdfs_gpu_index_remove(ctx._h, ix._h, p + 1, 16, r, f, None, None) == errno.EINVAL
        assert L.fdfs_gpu_index_lookup(ctx._h, ix._h, p + 1, 16, r, f, None) == errno.EINVAL
        assert L.fdfs_gpu_index_remove(ctx._h, ix._h, p, 16, None, f, None, None) == errno.EINVAL
        assert L.fdfs_gpu_index_lookup(ctx._h, ix._h, p, 16, None, f, None) == errno.EINVAL
        assert L.fdfs_gpu_index_remove(ctx._h, ix._h, p, 16, r, None, None, None) == errno.EINVAL
        assert L.fdfs_gpu_index_remove(ctx._h, ix._h, p, 16, r + 4, f, None, None) == errno.EINVAL
        assert L.fdfs_gpu_index_remove(ctx._h, ix._h, p, 0xFFFFFFFF, r, f, None, None) == errno.EINVAL
        assert L.fdfs_gpu_index_remove(ctx._h, ix._h, None, 0, None, None, None, None) == 0
        assert L.fdfs_gpu_index_tombstones(ix._h, None) == errno.EINVAL
        # unlink_out NULL is accepted
        assert L.fdfs_gpu_index_remove(ctx._h, ix._h, p, 16, r, f, None, None) == 0
        assert L.fdfs_gpu_index_lookup(ctx._h, ix._h, p, 16, r, f, None) == 0
        torch.cuda.synchronize()
        assert (rep == NONE).all() and (ref == 0).all()
        dead = ctypes.c_uint64(7)
        assert L.fdfs_gpu_index_tombstones(ix._h, ctypes.byref(dead)) == 0 and dead.value == 0
    finally:
        ix.close()


def test_lookup_replays_in_graph(ctx):
    """One lookup of a fixed tensor captured on one stream (a linear graph)
    and replayed as the index changes under it: each replay answers for the
    index of that moment.  The index is sized so that no ingest rehashes it
    (a captured call addresses the table it was captured on)."""
    from fastdfs_amd.api import DedupIndex
    present, absent = _distinct(600, 4001), _distinct(100, 4002)
    rng = np.random.default_rng(4003)
    q = np.concatenate([present, absent, present[rng.integers(0, 600, 300)]])
    q = q[rng.permutation(1000)]
    q_t = _dev(q)
    ctx.reserve(1000, 1000)
    ix, model = DedupIndex(ctx, 10_000), Model()
    try:
        s = torch.cuda.Stream()  # eager on a side stream first, as tests/test_gpu_graph.py does
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            rep, ref = ix.lookup(q_t)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        assert (rep == NONE).all() and (ref == 0).all()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = ix.lookup(q_t)

        def check():
            g.replay()
            torch.cuda.synchronize()
            mrep, mref = model.lookup(q)
            assert np.array_equal(out[0].cpu().numpy(), mrep)
            assert np.array_equal(out[1].cpu().numpy(), mref)
            return mrep

        _ingest(ix, model, np.concatenate([present, present[:200]]))
        assert int((check() == NONE).sum()) == 100
        _remove(ix, model, np.concatenate([present[:300], present[:200]]))  # half of them, whole classes
        assert int((check() == NONE).sum()) > 100 + 300
        assert ix.stats()["slots"] == 16384 and ix.stats()["tombstones"] == 300
    finally:
        ix.close()
