"""GPU: the output contract of the signature calls -- crc_out, sig_out and
codes_out on every kernel path that stores them, each of sig_out / codes_out
NULL, caller-owned outputs with guard bytes around them, the alignment
fdfs_gpu_sig_batch asks for, and fdfs_gpu_sig_batch_host's window planner on
batches that are not packed in increasing order.

One-shot batches (fdfs_gpu_sig_batch) store codes_out at these sites:

  1  sig_hash_kernel's lane epilogue        HASH  one int4
  2  elf_chain_wg                           HASH  codes[1] alone
  3  big_patch_kernel                       HASH  codes[0], [2], [3] alone
  4  md5_pair_kernel's lanes                MD5   the digest
  5  md5_chain_wg                           MD5   the digest
  6  md5_chain_wave                         MD5   the digest
  7  md5_stage_kernel<.., ST = false>       MD5   -- not reachable: see below

and the signature beside each of them by stores of its own.  Which site a
file reaches is decided by launch_sig_lane and big_plan_kernel (fdfs_sig.hip)
and the launchers (launch_sig_hash, launch_md5_stage).  With ncu compute
units and lat_files = 256 ncu, for a batch of n <= lat_files files whose
files >= 2^13 bytes all lie in [2^14, 2^14 + 512) (one size bin, upper bound
hi = 16,896) and whose other files are below 5,000 bytes (bin upper bound <=
5,120), big_plan_kernel compares, in 1/8 ps per byte,

    no offload                 hi * whole
    T = 2^14 (and 2^13: the same cost, ties go to the larger T)
                               max(5,120 * whole, hi * lean) + nbig * 2^14 * off
    T >= 2^15                  offloads nothing: the cost of no offload

    HASH  whole 168,000  lean 68,800  off 4:  1,162 M + nbig * 65,536 < 2,838 M
    MD5   whole 160,000  lean 92,000  off 2:  1,554 M + nbig * 32,768 < 2,703 M

so T = 2^14 for every nbig <= 4 ncu used here (nbig < 25,000), and the files
of 2^14 + r bytes are offloaded:

  "lanes"       133 files below 2^13 (no candidate T offloads anything):
                sites 1 and 4.
  "chain_wg"    40 big files <= ncu: each on a chain workgroup, elf_chain_wg
                (site 2) + big_patch_kernel (3), md5_chain_wg (5); the 61
                small files on the lanes.
  "chain_many"  ncu + 1 big files (> ncu, <= 4 ncu): HASH keeps their ELF on
                sig_hash_kernel's lanes in the offloaded form (the lane's int4
                store, then big_patch_kernel over codes 0 / 2 / 3: sites 1 +
                3), MD5 runs each on a wave (md5_chain_wave, site 6).

Site 7: launch_md5_stage starts md5_stage_kernel<.., false> only for a
one-shot batch without a queue, and launch_sig_lane, its one caller, always
passes the queue word of its workspace (hist + 2 kSizeBins), so every one-shot
MD5 batch takes md5_pair_kernel.  md5_stage_kernel's stores are the chunked
form's (states, no outputs); final_kernel's outputs are covered below and in
tests/test_gpu_state_resume.py.

Every reference value is oracle.dio_file's, file by file.
"""
import errno

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BIG = 1 << 14   # offloaded files are BIG + r bytes, r < 512: one size bin
GUARD = 4096    # bytes of 0xA5 on each side of a caller-owned output
FILL = 0xA5
SITES = ("lanes", "chain_wg", "chain_many")


@pytest.fixture(scope="module")
def ctxs():
    import fastdfs_amd as F
    if not torch.cuda.is_available():
        pytest.fail("gpu test collected without a GPU")
    return {0: F.Context(0, unsigned_hash=False), 1: F.Context(0, unsigned_hash=True)}


@pytest.fixture(scope="module")
def ncu(ctxs):
    return torch.cuda.get_device_properties(0).multi_processor_count


# ------------------------------------------------------------------ the shapes

def _sizes(site, ncu, rng):
    """The site's file sizes, with the premises of its path asserted."""
    if site == "lanes":
        edge = [0, 1, 55, 56, 63, 64, 65, 127, 128, 4031, 4095, 4097, 8191]
        sizes = np.concatenate([edge, rng.integers(0, 8192, 133 - len(edge))])
        assert sizes.size == 133 and sizes.size % 64 and sizes.max() < 1 << 13
        nbig = 0
    elif site == "chain_wg":
        nbig = 40
        assert nbig <= ncu, "a chain workgroup per big file needs at most one big file per CU"
        sizes = np.concatenate([BIG + rng.integers(0, 512, nbig), rng.integers(0, 5000, 60), [0]])
    elif site == "chain_many":
        nbig = ncu + 1
        assert ncu < nbig <= 4 * ncu
        sizes = np.concatenate([BIG + rng.integers(0, 512, nbig), rng.integers(0, 5000, 60)])
    else:  # n files of 100 bytes
        sizes = np.full(int(site[1:]), 100)
        nbig = 0
    sizes = sizes.astype(np.int64)
    big = sizes[sizes >= 1 << 13]  # smaller files are never offloaded (kMinLog)
    assert big.size == nbig and np.all((big >= BIG) & (big < BIG + 512))
    assert nbig == 0 or sizes[sizes < 1 << 13].max() < 5000
    assert sizes.size <= 256 * ncu  # big_plan_kernel picks T (n <= lat_files)
    rng.shuffle(sizes)
    return sizes


class _Shape:
    """A site's batch: host bytes, layout, the device copy, and the oracle's
    per-file results by (method, variant), each computed once."""

    def __init__(self, site, ncu):
        rng = np.random.default_rng(3000 + sum(site.encode()))
        self.sizes = _sizes(site, ncu, rng)
        self.n = self.sizes.size
        self.offs = np.zeros(self.n, np.int64)
        pos = 0
        for i, s in enumerate(self.sizes):
            pos += int(rng.integers(0, 16))  # files start at any byte
            self.offs[i] = pos
            pos += int(s)
        self.buf = rng.integers(0, 256, size=pos + 1, dtype=np.uint8)
        self.dev = tuple(torch.from_numpy(a).cuda() for a in (self.buf, self.offs, self.sizes))
        self._ref = {}

    def ref(self, o, method, variant):
        key = (method, variant)
        if key not in self._ref:
            self._ref[key] = _per_file(o, self.buf, self.offs, self.sizes, method, variant)
        return self._ref[key]


_shapes = {}


def _shape(site, ncu):
    if site not in _shapes:
        _shapes[site] = _Shape(site, ncu)
    return _shapes[site]


def _per_file(o, buf, offs, sizes, method, variant):
    """(crc uint32[n], sig uint8[n,24] | None, codes int32[n,4] | None) from
    oracle.dio_file on each file's own bytes."""
    n = len(sizes)
    crc = np.zeros(n, np.uint32)
    sig = np.zeros((n, 24), np.uint8) if method else None
    codes = np.zeros((n, 4), np.int32) if method else None
    for i in range(n):
        c, s, k = o.dio_file(buf[int(offs[i]): int(offs[i]) + int(sizes[i])], method, variant)
        crc[i] = c
        if method:
            sig[i] = np.frombuffer(s, np.uint8)
            codes[i] = k
    return crc, sig, codes


def _np(crc, sig, codes):
    torch.cuda.synchronize()
    return (crc.cpu().numpy().view(np.uint32), None if sig is None else sig.cpu().numpy(),
            None if codes is None else codes.cpu().numpy())


def _compare(got, want, sizes, tag):
    """crc, then the signature's six 4-byte fields, then the four codes: the
    failing files' sizes and how many files differ per field / column."""
    (crc, sig, codes), (wcrc, wsig, wcodes) = got, want
    bad = np.flatnonzero(crc != wcrc)
    assert bad.size == 0, (tag, "crc", bad[:10], sizes[bad[:10]])
    if wsig is not None and sig is not None:
        assert sig.shape == wsig.shape and sig.dtype == np.uint8
        bad = np.flatnonzero((sig != wsig).any(axis=1))
        fields = [int((sig[:, 4 * k: 4 * k + 4] != wsig[:, 4 * k: 4 * k + 4]).any(axis=1).sum()) for k in range(6)]
        assert bad.size == 0, (tag, "sig", bad[:10], sizes[bad[:10]], fields)
    if wcodes is not None and codes is not None:
        assert codes.shape == wcodes.shape and codes.dtype == np.int32
        bad = np.flatnonzero((codes != wcodes).any(axis=1))
        cols = [int((codes[:, k] != wcodes[:, k]).sum()) for k in range(4)]
        assert bad.size == 0, (tag, "codes", bad[:10], sizes[bad[:10]], cols)


# ------------------------------------------------- caller-owned outputs, guarded

class _Guarded:
    """An output as an interior slice of a larger tensor filled with 0xA5:
    GUARD bytes before it, the slice itself (pre-filled too, so an entry that
    is never written shows), GUARD bytes and the padding to 16 after it.
    `shift` moves the slice by that many bytes (the misalignment tests)."""

    def __init__(self, shape, dtype, shift=0):
        self.nbytes = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
        self.lo = GUARD + shift
        self.whole = torch.full((2 * GUARD + (self.nbytes + 15) // 16 * 16 + 16,), FILL, dtype=torch.uint8,
                                device="cuda")
        assert self.whole.data_ptr() % 16 == 0
        self.t = self.whole[self.lo: self.lo + self.nbytes].view(dtype).reshape(shape)
        assert self.t.is_contiguous() and self.t.data_ptr() == self.whole.data_ptr() + self.lo
        assert self.t.data_ptr() % 16 == shift % 16

    def outside(self):
        """True when every byte around the slice still holds the fill."""
        w = self.whole.cpu().numpy()
        return bool((w[: self.lo] == FILL).all() and (w[self.lo + self.nbytes:] == FILL).all())

    def untouched(self):
        return bool((self.whole.cpu().numpy() == FILL).all())


def _outputs(n, method, want_sig=True, want_codes=True, sig_shift=0, codes_shift=0):
    crc = _Guarded((n,), torch.int32)
    sig = _Guarded((n, 24), torch.uint8, sig_shift) if method and want_sig else None
    codes = _Guarded((n, 4), torch.int32, codes_shift) if method and want_codes else None
    return crc, sig, codes


def _call(ctx, dev, method, outs):
    crc, sig, codes = outs
    got = ctx.sig_batch(*dev, method=method, crc_out=crc.t, sig_out=None if sig is None else sig.t,
                        codes_out=None if codes is None else codes.t, want_sig=sig is not None,
                        want_codes=codes is not None)
    assert got[0] is crc.t and (sig is None) == (got[1] is None) and (codes is None) == (got[2] is None)
    return _np(*got)


# ----------------------------------------------------------------------- tests

@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("site", SITES)
def test_codes_every_path(oracle, ctxs, ncu, site, variant):
    """crc_out, sig_out and codes_out of each site's shape (module docstring)
    against oracle.dio_file file by file, HASH and MD5, both shift variants."""
    sh = _shape(site, ncu)
    for method in (1, 2):
        got = _np(*ctxs[variant].sig_batch(*sh.dev, method=method, want_codes=True))
        _compare(got, sh.ref(oracle, method, variant), sh.sizes, (site, method, variant))


@pytest.mark.parametrize("method", [1, 2])
@pytest.mark.parametrize("site", SITES)
def test_output_combinations(oracle, ctxs, ncu, site, method):
    """sig_out and codes_out each given or NULL (include/fdfs_gpu.h allows
    both): every site guards its two stores apart, so a guard that names the
    wrong pointer shows as an output left at its 0xA5 fill, or as a store
    through NULL.  All four calls give the oracle's CRCs, and every output
    that was asked for equals the oracle's and that of the (yes, yes) call."""
    sh = _shape(site, ncu)
    want = sh.ref(oracle, method, 0)
    full = None
    for want_sig, want_codes in ((True, True), (True, False), (False, True), (False, False)):
        outs = _outputs(sh.n, method, want_sig, want_codes)
        got = _call(ctxs[0], sh.dev, method, outs)
        assert (got[1] is not None) == want_sig and (got[2] is not None) == want_codes
        _compare(got, want, sh.sizes, (site, method, want_sig, want_codes))
        if full is None:
            full = got
        assert np.array_equal(got[0], full[0])
        assert got[1] is None or np.array_equal(got[1], full[1])
        assert got[2] is None or np.array_equal(got[2], full[2])


@pytest.mark.parametrize("method", [0, 1, 2])
@pytest.mark.parametrize("site", SITES + ("n1", "n63", "n64", "n65"))
def test_outputs_stay_inside_their_arrays(oracle, ctxs, ncu, site, method):
    """Caller-owned outputs inside larger tensors of 0xA5, 4,096 guard bytes
    on each side, the outputs pre-filled with 0xA5 as well: afterwards the
    guards are untouched and the outputs equal the oracle's, so every entry
    up to n - 1 was written and nothing beyond it.  Each site's shape (the
    last wave of every one is ragged) and n = 1, 63, 64, 65 files of 100
    bytes, a wave boundary +- 1."""
    sh = _shape(site, ncu)
    outs = _outputs(sh.n, method)
    got = _call(ctxs[0], sh.dev, method, outs)
    for name, g in zip(("crc_out", "sig_out", "codes_out"), outs):
        assert g is None or g.outside(), (site, method, name, "bytes around the output were written")
    _compare(got, sh.ref(oracle, method, 0), sh.sizes, (site, method))


@pytest.mark.parametrize("method", [0, 1, 2])
def test_final_batch_outputs_stay_inside(oracle, ctxs, method):
    """The same for fdfs_gpu_final_batch (final_kernel): 65 states, one
    update each, finalised through a permuted state_idx into guarded outputs:
    output i is state state_idx[i]'s."""
    rng = np.random.default_rng(3100 + method)
    n = 65
    sizes = np.concatenate([[0, 1, 55, 56, 63, 64, 65], rng.integers(0, 3000, n - 7)]).astype(np.int64)
    offs = np.zeros(n, np.int64)
    offs[1:] = np.cumsum(sizes + rng.integers(0, 16, n))[:-1]
    buf = rng.integers(0, 256, size=int(offs[-1] + sizes[-1]) + 1, dtype=np.uint8)
    ctx = ctxs[0]
    states = ctx.new_states(n)
    ctx.update_batch(states, *(torch.from_numpy(a).cuda() for a in (buf, offs, sizes)), method=method)
    perm = rng.permutation(n)
    outs = _outputs(n, method)
    crc, sig, codes = outs
    got = _np(*ctx.final_batch(states, method=method, state_idx=torch.from_numpy(perm.astype(np.int32)).cuda(),
                               want_codes=True, crc_out=crc.t, sig_out=None if sig is None else sig.t,
                               codes_out=None if codes is None else codes.t))
    for name, g in zip(("crc_out", "sig_out", "codes_out"), outs):
        assert g is None or g.outside(), (method, name, "bytes around the output were written")
    _compare(got, _per_file(oracle, buf, offs[perm], sizes[perm], method, 0), sizes[perm], ("final", method))


@pytest.mark.parametrize("method", [1, 2])
@pytest.mark.parametrize("which", ["sig+4", "codes+8", "codes+4", "crc+2"])
def test_misaligned_outputs_rejected(ctxs, ncu, which, method):
    """include/fdfs_gpu.h: crc_out 4-byte, sig_out 8-byte (uint2 stores),
    codes_out 16-byte (int4 stores) aligned, EINVAL otherwise -- checked
    before the lock and any launch, so nothing is written: every output
    tensor, guards and all, still holds its fill."""
    from fastdfs_amd.api import FdfsGpuError
    sh = _shape("n65", ncu)
    crc, sig, codes = _outputs(sh.n, method, sig_shift=4 if which == "sig+4" else 0,
                               codes_shift={"codes+8": 8, "codes+4": 4}.get(which, 0))
    crc_t = crc.t
    if which == "crc+2":
        crc_t = crc.whole[GUARD + 2: GUARD + 2 + 4 * sh.n]
    ptrs = (crc_t.data_ptr(), sig.t.data_ptr(), codes.t.data_ptr())
    assert (ptrs[0] % 4, ptrs[1] % 8, ptrs[2] % 16) == {"sig+4": (0, 4, 0), "codes+8": (0, 0, 8),
                                                        "codes+4": (0, 0, 4), "crc+2": (2, 0, 0)}[which]
    with pytest.raises(FdfsGpuError) as ei:
        ctxs[0].sig_batch(*sh.dev, method=method, crc_out=crc_t, sig_out=sig.t, codes_out=codes.t)
    assert ei.value.errno == errno.EINVAL
    torch.cuda.synchronize()
    assert crc.untouched() and sig.untouched() and codes.untouched()


# --------------------------------------------- the host-window planner's orders

_CHUNK = 64 << 10


def _host_layouts(rng):
    """name -> (offsets, sizes) over one 2 MB buffer, for 64 KiB windows."""
    lay = {}
    # (a) a gap larger than the window between two files: the second opens a
    # window of its own at or beyond lo + chunk
    lay["gap"] = ([1000, 31000 + (200 << 10), 31000 + (200 << 10) + 50000 + 3], [30000, 50000, 20000])
    # (b) packed files listed from the last to the first: every file starts
    # before the window of the one listed before it
    sz = rng.integers(0, 40000, 24)
    of = np.concatenate([[11], 11 + np.cumsum(sz + 5)[:-1]])
    lay["decreasing"] = (of[::-1], sz[::-1])
    # (c) the same byte range twice; two overlapping files in one window; two
    # overlapping files of which the first is split, so the second starts
    # before the window that holds the first one's rest
    lay["overlap"] = ([5000, 5000, 300000, 305000, 600000, 650000], [60000, 60000, 10000, 10000, 90000, 90000])
    # (d) exactly a window, a window + 1 byte, several windows: each first in
    # its window (the gaps are larger than a window)
    lay["window_sizes"] = ([7, 7 + _CHUNK + 70000, 7 + 2 * _CHUNK + 140001],
                           [_CHUNK, _CHUNK + 1, 300 << 10])
    # (e) empty files first, last, and around a split file and its neighbours
    # (an empty file has no piece, whatever its offset)
    lay["empties"] = ([0, 900000, 100, 0, 100100, 130100, 50, 130200, 230200, 0, 1999999],
                      [0, 0, 100000, 0, 30000, 0, 0, 100000, 0, 0, 0])
    # (f) nothing but empty files: no window at all
    lay["all_empty"] = ([0, 5, 1000000, 5, 0], [0, 0, 0, 0, 0])
    return {k: (np.asarray(o, np.int64), np.asarray(s, np.int64)) for k, (o, s) in lay.items()}


@pytest.mark.parametrize("method", [0, 1, 2])
def test_host_batch_orders(oracle, ctxs, method):
    """fdfs_gpu_sig_batch_host with 64 KiB windows on batches the header
    allows and plan_host_windows has branches for (fdfs_api.cpp): a file that
    starts at or beyond lo + chunk, files in decreasing offset order, files
    over identical and overlapping ranges, files of exactly a window, one
    byte more and several windows, empty files everywhere, only empty files.
    crc, sig and codes against oracle.dio_file on each file's own bytes (an
    overlapped range is hashed once per file, as the reference's per-file
    loop does)."""
    rng = np.random.default_rng(3200)
    buf = rng.integers(0, 256, size=2_000_000, dtype=np.uint8)
    for name, (offs, sizes) in _host_layouts(rng).items():
        assert int((offs + sizes).max()) <= buf.size
        crc, sig, codes = ctxs[0].sig_batch_host(buf, offs, sizes, method=method, want_codes=True,
                                                 chunk_bytes=_CHUNK)
        assert (sig is None) == (method == 0) and (codes is None) == (method == 0)
        _compare((crc, sig, codes), _per_file(oracle, buf, offs, sizes, method, 0), sizes, (name, method))
