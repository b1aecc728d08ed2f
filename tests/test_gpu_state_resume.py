"""GPU: fdfs_gpu_update_batch / final_batch on states the HOST wrote.

include/fdfs_gpu.h lays fdfs_gpu_file_state out "as StorageFileContext holds
it" and says a state "can be saved, moved between calls and streams, and
resumed".  Here every starting state is written by the oracle's host model
(oracle.FileState) from a real random prefix -- a state the reference could
hold, with stale bytes where the header leaves them unspecified (md5_buffer
past the pending count, reserved) -- uploaded, advanced by one GPU update, and
downloaded again: every field the header defines for the method (crc32,
hash_codes, md5_state, both count words, the pending md5_buffer bytes) equals
the model's, and final_batch equals the model's final.

Which kernel consumes the state depends on the batch's shape (launch_sig_lane
and big_plan_kernel, fdfs_sig.hip).  With ncu compute units:
  * chunks below 2^13 bytes are never offloaded: sig_hash_kernel's lanes
    (HASH), md5_stage_kernel's staged lanes (MD5);
  * a batch of n <= lat_files = 256 ncu chunks that all lie in [2^14, 2^14 +
    512) (one size bin, upper bound hi = 16,896) is offloaded at T = 2^14 when
    hi * lean + n * 2^14 * off < hi * whole, in 1/8 ps per byte
    (kLanePs * 8, kOffPs8):
      MD5   whole 160,000  lean 92,000  off 2:  n < 16,896 * 68,000 / 32,768 = 35,062
      HASH  whole 168,000  lean 68,800  off 4:  n < 16,896 * 99,200 / 65,536 = 25,574
    (T = 2^13 costs the same and ties go to the larger T; T >= 2^15 offloads
    nothing and costs `whole`); every batch here has at most 4 ncu chunks;
  * offloaded MD5 chunks: n <= ncu run md5_chain_wg (a workgroup each),
    ncu < n <= 4 ncu run md5_chain_wave (a wave each);
  * offloaded HASH chunks: n <= ncu run elf_chain_wg, n > ncu stay on
    sig_hash_kernel's lanes in their offloaded form (ELF alone);
  * both get crc32 (HASH: and hash_codes 0, 2, 3) from big_patch_state_kernel;
  * CRC only: crc_seg_kernel, then crc_carry_kernel.
"""
import hashlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BIG = 1 << 14  # offloaded chunk sizes are BIG + r, r < 512: one size bin


@pytest.fixture(scope="module")
def ctxs():
    import fastdfs_amd as F
    if not torch.cuda.is_available():
        pytest.fail("gpu test collected without a GPU")
    return {0: F.Context(0, unsigned_hash=False), 1: F.Context(0, unsigned_hash=True)}


@pytest.fixture(scope="module")
def ncu(ctxs):
    return torch.cuda.get_device_properties(0).multi_processor_count


def _bytes(rng, n, high=False):
    b = rng.integers(0, 256, size=int(n), dtype=np.uint8)
    return b | 0x80 if high else b


def _image(o, st, rng):
    """pack(st) with stale bytes where the header leaves them unspecified."""
    raw = np.frombuffer(o.pack(st), np.uint8).copy()
    at = 44 + (st.count & 63)
    raw[at:] = rng.integers(0, 256, size=128 - at, dtype=np.uint8)
    return raw


def _upload(o, models, rng):
    return torch.from_numpy(np.stack([_image(o, m, rng) for m in models])).cuda()


def _update(ctx, states, chunks, aligns, method, rng, sidx=None):
    """One update_batch call: chunk j at a byte offset = aligns[j] mod 16
    (random bytes between the chunks), onto states[sidx[j]] (default j)."""
    offs, pos = [], 0
    for c, a in zip(chunks, aligns):
        pos += (a - pos) % 16
        offs.append(pos)
        pos += len(c)
    buf = rng.integers(0, 256, size=pos + 16, dtype=np.uint8)
    for p0, c in zip(offs, chunks):
        buf[p0: p0 + len(c)] = c
    t = lambda x, dt: torch.tensor(x, dtype=dt, device="cuda")  # noqa: E731
    ctx.update_batch(states, torch.from_numpy(buf).cuda(), t(offs, torch.int64),
                     t([len(c) for c in chunks], torch.int64), method=method,
                     state_idx=None if sidx is None else t([int(s) for s in sidx], torch.int32))
    torch.cuda.synchronize()


_FIELDS = (("crc32", 0, 4), ("hash_codes", 4, 20), ("md5_state", 20, 36), ("md5_count", 36, 44),
           ("md5_buffer", 44, 108))


def _compare(o, ctx, states, models, method, tags):
    """Every defined field of the downloaded states, then final_batch,
    against the model."""
    got = states.cpu().numpy()
    exp = np.stack([np.frombuffer(o.pack(m), np.uint8) for m in models])
    mask = np.zeros(got.shape, bool)
    mask[:, 0:4] = mask[:, 36:44] = True
    if method == 1:
        mask[:, 4:20] = True
    if method == 2:
        mask[:, 20:36] = True
        for i, m in enumerate(models):
            mask[i, 44: 44 + (m.count & 63)] = True
    diff = (got != exp) & mask
    bad = np.flatnonzero(diff.any(axis=1))
    assert bad.size == 0, (len(bad), [(tags[i], [n for n, a, b in _FIELDS if diff[i, a:b].any()]) for i in bad[:5]])
    crc, sig, codes = ctx.final_batch(states, method=method, want_codes=True)
    torch.cuda.synchronize()
    crc = crc.cpu().numpy().view(np.uint32)
    if method:
        sig, codes = sig.cpu().numpy(), codes.cpu().numpy()
    for i, m in enumerate(models):
        wc, ws, wcodes = o.state_final(m, method)
        assert int(crc[i]) == wc, ("final crc", tags[i])
        if method:
            assert sig[i].tobytes() == ws, ("final sig", tags[i])
            assert [int(x) for x in codes[i]] == wcodes, ("final codes", tags[i])


def _split(n, most):
    """range(n) in the fewest near-equal calls of at most `most` chunks."""
    return np.array_split(np.arange(n), -(-n // most))


# ------------------------------------------------ (a) MD5 pending bytes, staged

@pytest.mark.parametrize("variant", [0, 1])
def test_md5_pending_grid_staged(oracle, ctxs, variant):
    """md5_stage_kernel<.., ST>: every (bytes pending, chunk length) pair in
    0..63 x 0..130, 8,384 states in one call (all chunks < 2^13: staged
    lanes).  The prefix holds 0, 1 or 2 whole blocks before the pending
    bytes, chunks sit at byte alignments cycling 0..15, state_idx is a random
    permutation.  The digest is also hashlib's over prefix || chunk."""
    o = oracle
    rng = np.random.default_rng(2100 + variant)
    grid = [(have, ln) for have in range(64) for ln in range(131)]
    prefixes = [_bytes(rng, have + 64 * (i % 3)) for i, (have, _) in enumerate(grid)]
    chunks = [_bytes(rng, ln) for _, ln in grid]
    models = [o.state_update(o.state_init(), p, 2, variant) for p in prefixes]
    assert sorted({m.count & 63 for m in models}) == list(range(64))
    states = _upload(o, models, rng)
    perm = rng.permutation(len(grid))
    _update(ctxs[variant], states, [chunks[s] for s in perm], [j % 16 for j in range(len(grid))], 2, rng, perm)
    for m, c in zip(models, chunks):
        o.state_update(m, c, 2, variant)
    _compare(o, ctxs[variant], states, models, 2, grid)
    for m, p, c, tag in zip(models, prefixes, chunks, grid):
        assert o.state_final(m, 2)[1][8:] == hashlib.md5(p.tobytes() + c.tobytes()).digest(), tag


# ------------------------------------------------- (b) MD5 pending bytes, chains

@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("path", ["md5_chain_wg", "md5_chain_wave"])
def test_md5_pending_grid_chains(oracle, ctxs, ncu, path, variant):
    """The two chain kernels' copies of the pending-byte logic: bytes pending
    0..63 x bytes left pending afterwards in {0, 1, 55, 56, 63} (55 / 56: the
    padding fits the block or not), 320 cases, chunks of 2^14 + r bytes, r <
    64.  Every call's chunks lie in one size bin at 2^14 and number far below
    35,062, so big_plan_kernel offloads them all (module docstring); calls of
    at most ncu chunks run md5_chain_wg, calls of ncu + 1 .. 4 ncu chunks run
    md5_chain_wave."""
    o = oracle
    rng = np.random.default_rng(2200 + variant)
    grid = [(have, left) for have in range(64) for left in (0, 1, 55, 56, 63)]
    if path == "md5_chain_wg":
        calls = _split(len(grid), ncu)
    else:
        grid = grid * -(-(ncu + 1) // len(grid))  # more cases than CUs
        calls = _split(len(grid), 4 * ncu)
        assert all(ncu < len(c) <= 4 * ncu for c in calls)
    prefixes = [_bytes(rng, have + 64 * (i % 2)) for i, (have, _) in enumerate(grid)]
    chunks = [_bytes(rng, BIG + (left - have) % 64) for have, left in grid]
    models = [o.state_update(o.state_init(), p, 2, variant) for p in prefixes]
    states = _upload(o, models, rng)
    for call in calls:
        perm = rng.permutation(call)
        _update(ctxs[variant], states, [chunks[s] for s in perm], [j % 16 for j in range(len(perm))], 2, rng, perm)
    for m, c, (_, left) in zip(models, chunks, grid):
        o.state_update(m, c, 2, variant)
        assert m.count & 63 == left
    _compare(o, ctxs[variant], states, models, 2, grid)


# --------------------------------------------------------------- (c) HASH resume

def _hash_cases(o, rng, lens_aligns, variant):
    """States after prefixes of 0..200 bytes, and their chunks; a share of
    both all >= 0x80 (ELFHash_ex's signed shift, CRC32_ex's signed state)."""
    prefixes = [_bytes(rng, i % 201, high=i % 3 == 0) for i in range(len(lens_aligns))]
    chunks = [_bytes(rng, ln, high=i % 5 == 0) for i, (ln, _) in enumerate(lens_aligns)]
    assert any((p >= 0x80).any() for p in prefixes) and any((c >= 0x80).any() for c in chunks)
    models = [o.state_update(o.state_init(), p, 1, variant) for p in prefixes]
    return models, chunks


@pytest.mark.parametrize("variant", [0, 1])
def test_hash_resume_lane(oracle, ctxs, variant):
    """sig_hash_kernel<.., ST>'s lanes: chunk lengths 0..130 x byte alignments
    0..15 in one call (no chunk reaches 2^13: nothing is offloaded), each
    onto a state the model wrote from a prefix of 0..200 bytes."""
    o = oracle
    rng = np.random.default_rng(2300 + variant)
    grid = [(ln, a) for ln in range(131) for a in range(16)]
    models, chunks = _hash_cases(o, rng, grid, variant)
    states = _upload(o, models, rng)
    _update(ctxs[variant], states, chunks, [a for _, a in grid], 1, rng)
    for m, c in zip(models, chunks):
        o.state_update(m, c, 1, variant)
    _compare(o, ctxs[variant], states, models, 1, grid)


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("path", ["elf_chain_wg", "offloaded_lane"])
def test_hash_resume_offloaded(oracle, ctxs, ncu, path, variant):
    """Offloaded HASH chunks, 2^14 + r bytes (r in 0..7) at alignments 0..3:
    far fewer than 25,574 chunks of one size bin per call, so all are
    offloaded (module docstring).  Calls of at most ncu chunks run
    elf_chain_wg; a call of more than ncu chunks keeps them on
    sig_hash_kernel's lanes (ELF alone).  crc32 and hash_codes 0, 2, 3 come
    from big_patch_state_kernel in both."""
    o = oracle
    rng = np.random.default_rng(2400 + variant)
    grid = [(BIG + r, a) for r in range(8) for a in range(4)]
    if path == "elf_chain_wg":
        calls = _split(len(grid), ncu)
    else:
        grid = grid * -(-(ncu + 1) // len(grid))
        calls = _split(len(grid), 4 * ncu)
        assert all(len(c) > ncu for c in calls)
    models, chunks = _hash_cases(o, rng, grid, variant)
    states = _upload(o, models, rng)
    for call in calls:
        perm = rng.permutation(call)
        _update(ctxs[variant], states, [chunks[s] for s in perm], [grid[s][1] for s in perm], 1, rng, perm)
    for m, c in zip(models, chunks):
        o.state_update(m, c, 1, variant)
    _compare(o, ctxs[variant], states, models, 1, grid)


# ------------------------------------------------ (d) count carries, every path

_BASES = [(1 << 29) - 64,  # the chunk crosses 2^32 bits: md5_count[0] carries into [1]
          (1 << 32) - 64,  # the size crosses 4 GiB: the high word of the signature's be64 size
          1 << 40]         # a large high word, no crossing
# path -> (method, chunks per call): "small" chunks of 65..200 bytes, "few"
# (<= ncu) or "many" (ncu + 1) offloaded chunks of 2^14 + r bytes
_CARRY_PATHS = {"crc_carry_kernel": (0, "small"), "hash_lane": (1, "small"), "hash_offloaded_lane": (1, "many"),
                "elf_chain_wg": (1, "few"), "md5_staged": (2, "small"), "md5_chain_wave": (2, "many"),
                "md5_chain_wg": (2, "few")}


@pytest.mark.parametrize("path", list(_CARRY_PATHS))
def test_count_carries(oracle, ctxs, ncu, path):
    """count_add at each of its six call sites (sig_hash_kernel's serves two
    paths).  The byte counts are set with virtual_prefix on states whose
    words come from a real prefix of 0..63 bytes, so a few KiB of data reach
    counts that need gigabytes of real bytes.  Against the model: both count
    words, the signature's size field, the MD5 digest (its padding carries
    both count words) and the CRC, for both variants."""
    o = oracle
    method, shape = _CARRY_PATHS[path]
    n = {"small": 12, "few": min(6, ncu), "many": ncu + 1}[shape]
    for variant in (0, 1):
        rng = np.random.default_rng(2500 + variant)
        bases = [_BASES[i % 3] for i in range(n)]
        plens = [(11 * i + 1) % 64 for i in range(n)]
        chunks = [_bytes(rng, 65 + 9 * i if shape == "small" else BIG + i % 64) for i in range(n)]
        models = [o.virtual_prefix(o.state_update(o.state_init(), _bytes(rng, p), method, variant), b // 64)
                  for p, b in zip(plens, bases)]
        before = [m.count for m in models]
        states = _upload(o, models, rng)
        perm = rng.permutation(n)
        _update(ctxs[variant], states, [chunks[s] for s in perm], [j % 16 for j in range(n)], method, rng, perm)
        for m, c in zip(models, chunks):
            o.state_update(m, c, method, variant)
        # the model's counts do what each base is there for
        for m, b0, base in zip(models, before, bases):
            lo0, hi0, lo1, hi1 = 8 * b0 & 0xFFFFFFFF, 8 * b0 >> 32, 8 * m.count & 0xFFFFFFFF, 8 * m.count >> 32
            if base == _BASES[0]:
                assert (hi0, hi1) == (0, 1) and lo1 < lo0
            elif base == _BASES[1]:
                assert b0 < 1 << 32 <= m.count and (hi0, hi1) == (7, 8)
            else:
                assert hi0 == hi1 == 2048
            if method:
                assert int.from_bytes(o.state_final(m, method)[1][:8], "big") == m.count
        _compare(o, ctxs[variant], states, models, method, list(zip(bases, plens)))


# ------------------------------------------------------ (e) handover both ways

def _splits(rng, size, small_frac=0.3, max_chunk=70_000):
    """Random cut points of one file, as tests/test_gpu_stream.py cuts them:
    tiny (<= 63, MD5 tail fills), zero-length and 1..max_chunk byte chunks."""
    cuts, pos = [], 0
    while pos < size:
        step = int(rng.integers(0, 64)) if rng.random() < small_frac else int(rng.integers(1, max_chunk))
        step = min(step, size - pos)
        cuts.append(step)
        pos += step
    if not cuts or rng.random() < 0.2:
        cuts.append(0)
    return cuts


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("method", [0, 1, 2])
def test_handover_gpu_and_host(oracle, ctxs, method, variant):
    """Three files of about 300 KB move between the GPU and the host model
    chunk by chunk: chunk k is applied by update_batch when k is even, and
    when k is odd the state is downloaded, unpacked, advanced by the model,
    packed and uploaded; a second pass swaps the parities (its first chunk
    goes onto fdfs_gpu_state_init's state, read by the host).  Both
    final_batch and the model's final of the downloaded state equal the
    oracle's one-shot values."""
    o = oracle
    ctx = ctxs[variant]
    rng = np.random.default_rng(2600 + 10 * method + variant)
    files = [_bytes(rng, s) for s in (299_999, 300_037, 310_001)]
    want = [o.dio_file(f, method, variant) for f in files]
    for gpu_parity in (0, 1):
        cuts = [_splits(rng, len(f)) for f in files]
        states = ctx.new_states(len(files))
        pos = [0] * len(files)
        on_gpu = on_host = 0
        for k in range(max(len(c) for c in cuts)):
            live = [i for i in range(len(files)) if k < len(cuts[i])]
            parts = [files[i][pos[i]: pos[i] + cuts[i][k]] for i in live]
            if k % 2 == gpu_parity:
                _update(ctx, states, parts, [int(a) for a in rng.integers(0, 16, len(live))], method, rng, live)
                on_gpu += 1
            else:
                rows = states.cpu().numpy()
                for i, part in zip(live, parts):
                    rows[i] = _image(o, o.state_update(o.unpack(rows[i]), part, method, variant), rng)
                states.copy_(torch.from_numpy(rows))
                on_host += 1
            for i in live:
                pos[i] += cuts[i][k]
        assert pos == [len(f) for f in files] and on_gpu > 2 and on_host > 2
        crc, sig, codes = ctx.final_batch(states, method=method, want_codes=True)
        torch.cuda.synchronize()
        rows = states.cpu().numpy()
        crc = crc.cpu().numpy().view(np.uint32)
        if method:
            sig, codes = sig.cpu().numpy(), codes.cpu().numpy()
        for i in range(len(files)):
            got = (int(crc[i]), sig[i].tobytes() if method else None,
                   [int(x) for x in codes[i]] if method else None)
            assert got == want[i], (gpu_parity, i)
            assert o.state_final(o.unpack(rows[i]), method) == want[i], (gpu_parity, i)


# --------------------------------------------------- (f) crc_combine, large |B|

@pytest.mark.parametrize("variant", [0, 1])
def test_crc_combine_large_lengths(oracle, ctxs, variant):
    """fdfs_gpu_crc_combine with |B| around 2^32, at 2^40 + 12,345 and at the
    documented bound 2^48 - 1, random crc_a / crc_b, bit-exact against the
    GF(2) square-and-multiply of oracle.crc32_combine (checked against real
    zero runs in tests/test_state_model.py)."""
    rng = np.random.default_rng(2700 + variant)
    lens = [(1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 40) + 12345, (1 << 48) - 1]
    cases = [(int(a), int(b), n) for n in lens for a, b in rng.integers(0, 1 << 32, size=(6, 2))]
    cases += [(1 << i, 0, lens[-1]) for i in (0, 31)]
    t32 = lambda x: torch.from_numpy(np.array(x, np.uint32).view(np.int32)).cuda()  # noqa: E731
    out = ctxs[variant].crc_combine(t32([c[0] for c in cases]), t32([c[1] for c in cases]),
                                    torch.tensor([c[2] for c in cases], dtype=torch.int64, device="cuda"))
    got = [int(x) for x in out.cpu().numpy().view(np.uint32)]
    assert got == [oracle.crc32_combine(a, b, n, variant) for a, b, n in cases]
