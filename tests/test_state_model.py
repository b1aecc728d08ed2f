"""CPU: the oracle's host model of fdfs_gpu_file_state (oracle.FileState:
state_init / state_update / state_final / pack / unpack / virtual_prefix) and
its pure-Python crc32_combine, checked against the oracle's one-shot values,
hashlib and real zero runs.  tests/test_gpu_state_resume.py then uses both as
the reference for states the GPU resumes.
"""
import hashlib

import numpy as np
import pytest


def _chunks(rng, size):
    """Random cuts: tiny (MD5 tail fills), empty and large chunks."""
    cuts, pos = [], 0
    while pos < size:
        step = int(rng.integers(0, 64)) if rng.random() < 0.4 else int(rng.integers(1, 5000))
        step = min(step, size - pos)
        cuts.append(step)
        pos += step
    return cuts + [0]


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("method", [0, 1, 2])
def test_model_in_chunks_equals_one_shot(oracle, method, variant):
    rng = np.random.default_rng(900 + 10 * method + variant)
    for size in [0, 1, 63, 64, 65, 127, 128, 1000, 20_011, 70_000]:
        f = rng.integers(0, 256, size=size, dtype=np.uint8)
        st = oracle.state_init()
        pos = 0
        for c in _chunks(rng, size):
            oracle.state_update(st, f[pos: pos + c], method, variant)
            pos += c
            assert st.count == pos
            if method == 1:
                assert st.h[0] == st.crc
            if method == 2:
                assert st.pending == f[pos - pos % 64: pos].tobytes()
        want = oracle.dio_file(f, method, variant)
        assert oracle.state_final(st, method) == want, size
        # final leaves the state as it is: a second final agrees
        assert oracle.state_final(st, method) == want, size
        if method == 2:
            assert want[1][8:] == hashlib.md5(f.tobytes()).digest()
            assert int.from_bytes(want[1][:8], "big") == size


@pytest.mark.parametrize("method", [0, 1, 2])
def test_pack_unpack_round_trip(oracle, method):
    rng = np.random.default_rng(40 + method)
    for size in [0, 5, 64, 100, 6000]:
        f = rng.integers(0, 256, size=size, dtype=np.uint8)
        st = oracle.state_update(oracle.state_init(), f, method, 0)
        raw = oracle.pack(st)
        assert len(raw) == oracle.FILE_STATE_SIZE == 128
        back = oracle.unpack(raw)
        for m in (0, 1, 2):
            assert back.fields(m) == st.fields(m)
        assert oracle.pack(back) == raw
        # bytes the GPU leaves unspecified do not reach the model
        dirty = np.frombuffer(raw, np.uint8).copy()
        dirty[44 + size % 64: 108] ^= 0xA5
        dirty[108:] = 0x5A
        assert oracle.pack(oracle.unpack(dirty)) == raw
        # and the resumed state goes on as the original does
        more = rng.integers(0, 256, size=777, dtype=np.uint8)
        assert oracle.state_final(oracle.state_update(oracle.unpack(dirty), more, method, 0), method) == \
            oracle.dio_file(np.concatenate([f, more]), method, 0)


def test_pack_layout(oracle):
    """The image's fields sit where include/fdfs_gpu.h puts them
    (test_abi.py pins those offsets): count in bits, low word first."""
    f = np.arange(70, dtype=np.uint8)
    st = oracle.state_update(oracle.state_init(), f, 2, 0)
    oracle.virtual_prefix(st, 1 << 26)  # + 2^32 bytes: bit 35 of the bit count
    raw = np.frombuffer(oracle.pack(st), np.uint8)
    assert int(raw[0:4].view(np.int32)[0]) == oracle.crc32_ex(f, -1, 0)
    assert [int(x) for x in raw[4:20].view(np.int32)] == [-1, 0, 0, 0]
    assert [int(x) for x in raw[36:44].view(np.uint32)] == [8 * 70, 8]
    assert raw[44:50].tobytes() == f[64:].tobytes()
    assert not raw[50:].any()


def test_virtual_prefix_changes_the_count_alone(oracle):
    rng = np.random.default_rng(8)
    f = rng.integers(0, 256, size=100, dtype=np.uint8)
    for method in (0, 1, 2):
        st = oracle.state_update(oracle.state_init(), f, method, 0)
        vp = oracle.virtual_prefix(st.copy(), 3)
        assert vp.count == st.count + 192
        assert vp.fields(method)[0] == st.fields(method)[0]
        assert vp.fields(method)[2:] == st.fields(method)[2:]
    # 192 real zero bytes hashed first give the same count, and for MD5 the
    # digest differs only through the state words: the padding is the same
    real = oracle.state_update(oracle.state_init(), np.concatenate([np.zeros(192, np.uint8), f]), 2, 0)
    assert real.count == vp.count and real.pending == vp.pending


@pytest.mark.slow
def test_md5_count_carry_real_bytes(oracle):
    """The oracle's own carry into the high count word, pinned with real
    bytes: MD5 over 512 MiB + 100 zero bytes (2^32 + 800 bits) against
    hashlib, both fed from one 1 MiB buffer."""
    buf = np.zeros(1 << 20, np.uint8)
    raw = buf.tobytes()
    h = hashlib.md5()
    st = oracle.state_init()
    for _ in range(512):
        h.update(raw)
        oracle.state_update(st, buf, 2, 0)
    h.update(raw[:100])
    oracle.state_update(st, buf[:100], 2, 0)
    assert st.count == (512 << 20) + 100
    assert [int(x) for x in np.frombuffer(oracle.pack(st), np.uint8)[36:44].view(np.uint32)] == [800, 1]
    crc, sig, _ = oracle.state_final(st, 2)
    assert sig[8:] == h.digest()
    assert int.from_bytes(sig[:8], "big") == st.count
    # the same count reached by virtual_prefix over these state words: the
    # padding and size field come out the same
    vp = st.copy()
    vp.md5.count = 100
    assert oracle.state_final(vp, 2)[1] != sig
    assert oracle.state_final(oracle.virtual_prefix(vp, 1 << 23), 2) == (crc, sig, _)


@pytest.mark.parametrize("variant", [0, 1])
def test_crc_combine_reference_vs_zero_runs(oracle, variant):
    """The GF(2) square-and-multiply equals CRC32_ex over real zero bytes, and
    joins two pieces by the identity of include/fdfs_gpu.h."""
    rng = np.random.default_rng(17 + variant)
    for n in [0, 1, 255, 65_537, 1 << 20]:
        z = np.zeros(n, np.uint8)
        for v in [1, 0x80000000, 0xFFFFFFFF] + [int(x) for x in rng.integers(0, 1 << 32, 3)]:
            assert oracle.crc_zero_advance(v, n, variant) == oracle.crc32_ex(z, v, variant) & 0xFFFFFFFF, (n, v)
        assert oracle.crc_zero_advance(0, n, variant) == 0
        a = rng.integers(0, 256, size=int(rng.integers(1, 3000)), dtype=np.uint8)
        b = rng.integers(0, 256, size=n, dtype=np.uint8)
        crc_a, crc_b = oracle.crc32_ex(a, -1, variant), oracle.crc32_ex(b, 0, variant)
        assert crc_a & 0xFFFFFFFF and (n == 0 or crc_b & 0xFFFFFFFF)
        assert oracle.crc32_combine(crc_a, crc_b, n, variant) == \
            oracle.crc32_ex(np.concatenate([a, b]), -1, variant) & 0xFFFFFFFF, n
