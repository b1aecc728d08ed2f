"""ctypes wrapper over the C oracle (oracle/fdfs_oracle.c).

TEST INFRASTRUCTURE ONLY: imported by tests/, __graft_entry__.smoke() and
bench.py's cpu_baseline leg, always as the checker / CPU baseline and never
as the thing measured or shipped.  The product library (libfdfs_gpu) does not
link or call any of this.

Parity status: MD5 pinned by RFC 1321 vectors; the unsigned CRC32 variant
pinned by zlib; the signed (libfastcommon-as-declared) CRC32/ELF variant is
PARITY UNPINNED -- libfastcommon is not vendored in the reference and no
reference test pins a value ("Oracle").
"""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "build", "liboracle.so")

VARIANT_SIGNED = 0
VARIANT_UNSIGNED = 1
METHOD_CRC_ONLY = 0
METHOD_HASH = 1
METHOD_MD5 = 2
FILE_SIG_SIZE = 24

_lib = None


def build() -> str:
    subprocess.run(["make", "-s", "-C", _HERE], check=True)
    return _SO


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(_SO):
            build()
        L = ctypes.CDLL(_SO)
        u8p = ctypes.c_void_p
        L.orc_crc32_ex.restype = ctypes.c_int32
        L.orc_crc32_ex.argtypes = [u8p, ctypes.c_size_t, ctypes.c_int32, ctypes.c_int]
        L.orc_crc32_final.restype = ctypes.c_int32
        L.orc_crc32_final.argtypes = [ctypes.c_int32]
        L.orc_elf_ex.restype = ctypes.c_int32
        L.orc_elf_ex.argtypes = [u8p, ctypes.c_size_t, ctypes.c_int32, ctypes.c_int]
        L.orc_simple_ex.restype = ctypes.c_int32
        L.orc_simple_ex.argtypes = [u8p, ctypes.c_size_t, ctypes.c_int32]
        L.orc_time33_ex.restype = ctypes.c_int32
        L.orc_time33_ex.argtypes = [u8p, ctypes.c_size_t, ctypes.c_int32]
        L.orc_crc_table_entry.restype = ctypes.c_uint32
        L.orc_crc_table_entry.argtypes = [ctypes.c_int]
        L.orc_dio_file.restype = None
        L.orc_dio_file.argtypes = [u8p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int,
                                   ctypes.c_int, u8p, u8p, u8p]
        L.orc_dio_batch.restype = ctypes.c_int
        L.orc_dio_batch.argtypes = [u8p, u8p, u8p, ctypes.c_uint64, ctypes.c_size_t,
                                    ctypes.c_int, ctypes.c_int, u8p, u8p, ctypes.c_int]
        L.orc_gen_files_total.restype = ctypes.c_uint64
        L.orc_gen_files.restype = None
        L.orc_gen_files.argtypes = [u8p]
        L.orc_dedup.restype = ctypes.c_int
        L.orc_dedup.argtypes = [u8p, ctypes.c_uint64, u8p, u8p]
        L.orc_dedup_mt.restype = ctypes.c_int
        L.orc_dedup_mt.argtypes = [u8p, ctypes.c_uint64, u8p, u8p, ctypes.c_int]
        L.orc_md5_init.argtypes = [u8p]
        L.orc_md5_update.argtypes = [u8p, u8p, ctypes.c_size_t]
        L.orc_md5_final.argtypes = [u8p, u8p]
        L.orc_sig_pack.restype = None
        L.orc_sig_pack.argtypes = [ctypes.c_int64, ctypes.c_int, u8p, u8p]
        _lib = L
    return _lib


def _ptr(a: np.ndarray) -> int:
    return a.ctypes.data


def _u8(data) -> np.ndarray:
    if isinstance(data, (bytes, bytearray, memoryview)):
        return np.frombuffer(bytes(data), dtype=np.uint8)
    return np.ascontiguousarray(data, dtype=np.uint8)


def crc32_ex(data, init: int = -1, variant: int = VARIANT_SIGNED) -> int:
    a = _u8(data)
    return lib().orc_crc32_ex(_ptr(a), a.size, ctypes.c_int32(init).value, variant)


def crc32(data, variant: int = VARIANT_SIGNED) -> int:
    """CRC32_XINIT -> CRC32_ex -> CRC32_FINAL, as an unsigned 32-bit value
    (what fdfs_crc32 prints with %u, client/fdfs_crc32.c:100)."""
    return lib().orc_crc32_final(crc32_ex(data, -1, variant)) & 0xFFFFFFFF


def elf_ex(data, init: int = 0, variant: int = VARIANT_SIGNED) -> int:
    a = _u8(data)
    return lib().orc_elf_ex(_ptr(a), a.size, init, variant)


def simple_ex(data, init: int = 0) -> int:
    a = _u8(data)
    return lib().orc_simple_ex(_ptr(a), a.size, init)


def time33_ex(data, init: int = 0) -> int:
    a = _u8(data)
    return lib().orc_time33_ex(_ptr(a), a.size, init)


def md5(data) -> bytes:
    a = _u8(data)
    ctx = ctypes.create_string_buffer(128)
    out = ctypes.create_string_buffer(16)
    L = lib()
    L.orc_md5_init(ctypes.addressof(ctx))
    L.orc_md5_update(ctypes.addressof(ctx), _ptr(a), a.size)
    L.orc_md5_final(ctypes.addressof(out), ctypes.addressof(ctx))
    return out.raw


def dio_file(data, method: int, variant: int = VARIANT_SIGNED, chunk: int = 256 * 1024):
    """Returns (crc32 unsigned, sig24 bytes or None, hash codes (4 int32) or None)."""
    a = _u8(data)
    crc = np.zeros(1, np.uint32)
    sig = np.zeros(24, np.uint8)
    codes = np.zeros(4, np.int32)
    lib().orc_dio_file(_ptr(a), a.size, chunk, method, variant, _ptr(crc), _ptr(sig),
                       _ptr(codes))
    if method == METHOD_CRC_ONLY:
        return int(crc[0]), None, None
    return int(crc[0]), sig.tobytes(), [int(x) for x in codes]


def dio_batch(base: np.ndarray, offset: np.ndarray, size: np.ndarray, method: int,
              variant: int = VARIANT_SIGNED, chunk: int = 256 * 1024, nthreads: int = 1):
    """Oracle over a batch; returns (crc uint32[n], sig uint8[n,24])."""
    base = np.ascontiguousarray(base, dtype=np.uint8)
    offset = np.ascontiguousarray(offset, dtype=np.uint64)
    size = np.ascontiguousarray(size, dtype=np.uint64)
    n = offset.size
    crc = np.zeros(n, np.uint32)
    sig = np.zeros((n, 24), np.uint8)
    rc = lib().orc_dio_batch(_ptr(base), _ptr(offset), _ptr(size), n, chunk, method, variant,
                             _ptr(crc), _ptr(sig), nthreads)
    assert rc == 0
    return crc, sig


def codes_from_sig(sig: np.ndarray, method: int) -> np.ndarray:
    """int32[n,4]: the codes StorageFileContext holds for signatures
    uint8[n,24] (dio_batch's): HASH, the four big-endian fields at bytes
    8..24 (int2buff of file_hash_codes after FINISH); MD5, bytes 8..24 as
    little-endian words (the digest is the state words stored little-endian,
    which orc_dio_file copies into codes).  tests/test_oracle.py ties it to
    dio_file's codes."""
    assert method in (METHOD_HASH, METHOD_MD5)
    sig = np.ascontiguousarray(sig, dtype=np.uint8).reshape(-1, FILE_SIG_SIZE)
    words = np.ascontiguousarray(sig[:, 8:]).view(">u4" if method == METHOD_HASH else "<u4")
    return words.astype(np.uint32).view(np.int32).reshape(-1, 4)


# ---- host model of fdfs_gpu_file_state (include/fdfs_gpu.h) ----------------
# The per-upload state StorageFileContext carries between chunks
# (storage/storage_nio.h:94-96), advanced with the oracle's own primitives, and
# its 128-byte image as the GPU library lays it out.  Tests write states with
# it, upload them, and compare what the kernels leave with what it holds.

FILE_STATE_SIZE = 128
_ST_CRC, _ST_CODES, _ST_MD5, _ST_COUNT, _ST_BUF, _ST_RESERVED = 0, 4, 20, 36, 44, 108


class _Md5Ctx(ctypes.Structure):  # orc_md5_ctx
    _fields_ = [("state", ctypes.c_uint32 * 4), ("count", ctypes.c_uint64),
                ("buffer", ctypes.c_uint8 * 64)]


class FileState:
    """crc: CRC32_ex running value (int32); h: file_hash_codes (4 int32);
    md5: orc_md5_ctx, whose count (bytes) is kept for every method."""
    __slots__ = ("crc", "h", "md5")

    @property
    def count(self) -> int:
        return int(self.md5.count)

    @property
    def pending(self) -> bytes:
        """The (count % 64) bytes my_md5_update holds back."""
        return bytes(self.md5.buffer[: self.count & 63])

    def copy(self) -> "FileState":
        st = FileState()
        st.crc, st.h = self.crc, list(self.h)
        st.md5 = _Md5Ctx.from_buffer_copy(self.md5)
        return st

    def fields(self, method: int) -> tuple:
        """The fields include/fdfs_gpu.h defines for `method`, comparable."""
        out = (self.crc, self.count)
        if method == METHOD_HASH:
            out += (tuple(self.h),)
        elif method == METHOD_MD5:
            out += (tuple(self.md5.state), self.pending)
        return out


def state_init() -> FileState:
    """storage_write_to_file: CRC32_XINIT, INIT_HASH_CODES4, my_md5_init."""
    st = FileState()
    st.crc = -1
    st.h = [-1, 0, 0, 0]
    st.md5 = _Md5Ctx()
    lib().orc_md5_init(ctypes.addressof(st.md5))
    return st


def state_update(st: FileState, data, method: int, variant: int = VARIANT_SIGNED) -> FileState:
    """dio_write_file's update for one chunk, in place: CRC32_ex always,
    CALC_HASH_CODES4 for HASH, my_md5_update for MD5, the byte count always."""
    a = _u8(data)
    st.crc = crc32_ex(a, st.crc, variant)
    if method == METHOD_HASH:
        st.h = [crc32_ex(a, st.h[0], variant), elf_ex(a, st.h[1], variant),
                simple_ex(a, st.h[2]), time33_ex(a, st.h[3])]
    if method == METHOD_MD5:
        lib().orc_md5_update(ctypes.addressof(st.md5), _ptr(a), a.size)
    else:
        st.md5.count += a.size
    return st


def state_final(st: FileState, method: int):
    """dio_write_file's finalisation, as dio_file returns it: (crc32 unsigned,
    sig24 or None, codes or None).  st is left as it is."""
    L = lib()
    crc = L.orc_crc32_final(st.crc) & 0xFFFFFFFF
    if method == METHOD_CRC_ONLY:
        return crc, None, None
    codes = np.zeros(4, np.int32)
    if method == METHOD_HASH:
        codes[:] = [L.orc_crc32_final(st.h[0])] + st.h[1:]  # FINISH_HASH_CODES4
    else:
        ctx = _Md5Ctx.from_buffer_copy(st.md5)
        L.orc_md5_final(_ptr(codes), ctypes.addressof(ctx))
    sig = np.zeros(24, np.uint8)
    L.orc_sig_pack(st.count, method, _ptr(codes), _ptr(sig))
    return crc, sig.tobytes(), [int(x) for x in codes]


def virtual_prefix(st: FileState, k: int) -> FileState:
    """As if 64 k more bytes had gone before: the byte count alone rises, in
    place.  None of the recurrences reads the count (only MD5's final padding
    and the signature's size field do), and a multiple of 64 leaves the
    pending bytes where they are."""
    st.md5.count += 64 * k
    return st


def pack(st: FileState) -> bytes:
    """The state as fdfs_gpu_file_state (128 bytes): count in bits, low word
    first; buffer bytes past the pending ones and `reserved` are zero."""
    out = np.zeros(FILE_STATE_SIZE, np.uint8)
    out[_ST_CRC:_ST_CODES].view(np.int32)[0] = st.crc
    out[_ST_CODES:_ST_MD5].view(np.int32)[:] = st.h
    out[_ST_MD5:_ST_COUNT].view(np.uint32)[:] = list(st.md5.state)
    out[_ST_COUNT:_ST_BUF].view(np.uint32)[:] = [(8 * st.count) & 0xFFFFFFFF, (8 * st.count) >> 32 & 0xFFFFFFFF]
    pend = st.pending
    out[_ST_BUF:_ST_BUF + len(pend)] = np.frombuffer(pend, np.uint8)
    return out.tobytes()


def unpack(raw) -> FileState:
    """The model of a 128-byte fdfs_gpu_file_state.  Buffer bytes past the
    pending count and `reserved` are unspecified there and are dropped."""
    a = _u8(raw)
    assert a.size == FILE_STATE_SIZE
    st = FileState()
    st.crc = int(a[_ST_CRC:_ST_CODES].view(np.int32)[0])
    st.h = [int(x) for x in a[_ST_CODES:_ST_MD5].view(np.int32)]
    st.md5 = _Md5Ctx()
    for i, x in enumerate(a[_ST_MD5:_ST_COUNT].view(np.uint32)):
        st.md5.state[i] = int(x)
    lo, hi = (int(x) for x in a[_ST_COUNT:_ST_BUF].view(np.uint32))
    st.md5.count = (hi << 32 | lo) >> 3
    for i in range(st.count & 63):
        st.md5.buffer[i] = int(a[_ST_BUF + i])
    return st


# ---- crc32_combine over GF(2), in plain Python ------------------------------

def crc_zero_advance(v: int, nbytes: int, variant: int = VARIANT_SIGNED) -> int:
    """M^nbytes v, M the CRC32_ex step over one zero byte (a linear map of the
    32-bit state for both shift variants): square-and-multiply on M's columns,
    which are CRC32_ex(b"\\0", 1 << i).  Unsigned 32-bit in and out."""
    zero = np.zeros(1, np.uint8)
    m = [crc32_ex(zero, 1 << i, variant) & 0xFFFFFFFF for i in range(32)]

    def apply(cols, x):
        r = 0
        for i in range(32):
            if x >> i & 1:
                r ^= cols[i]
        return r

    v &= 0xFFFFFFFF
    while nbytes:
        if nbytes & 1:
            v = apply(m, v)
        m = [apply(m, c) for c in m]
        nbytes >>= 1
    return v


def crc32_combine(crc_a: int, crc_b: int, len_b: int, variant: int = VARIANT_SIGNED) -> int:
    """CRC32_ex(A || B, init) from crc_a = CRC32_ex(A, init), crc_b =
    CRC32_ex(B, 0) and len_b = |B| (include/fdfs_gpu.h, fdfs_gpu_crc_combine)."""
    return crc_zero_advance(crc_a, len_b, variant) ^ (crc_b & 0xFFFFFFFF)


def gen_files() -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """test/gen_files.c corpus: (bytes, offsets, sizes) of the 6 files."""
    L = lib()
    total = L.orc_gen_files_total()
    buf = np.empty(total, np.uint8)
    L.orc_gen_files(_ptr(buf))
    sizes = np.array([5 << 10, 50 << 10, 200 << 10, 1 << 20, 10 << 20, 100 << 20], np.uint64)
    offs = np.zeros(6, np.uint64)
    offs[1:] = np.cumsum(sizes)[:-1]
    return buf, offs, sizes


def dedup(sig: np.ndarray, nthreads: int = 1, partitioned: bool = False) -> tuple[np.ndarray, np.ndarray]:
    """(rep uint64[n], ref uint32[n]) with the sequential FastDHT semantics
    (nthreads > 1 or partitioned: the hash-partitioned form, same answers)."""
    sig = np.ascontiguousarray(sig, dtype=np.uint8).reshape(-1, 24)
    n = sig.shape[0]
    rep = np.zeros(n, np.uint64)
    ref = np.zeros(n, np.uint32)
    if nthreads > 1 or partitioned:
        assert lib().orc_dedup_mt(_ptr(sig), n, _ptr(rep), _ptr(ref), nthreads) == 0
    else:
        assert lib().orc_dedup(_ptr(sig), n, _ptr(rep), _ptr(ref)) == 0
    return rep, ref


# ---- formats that consume the CRC, FastDHT routing ----------

def _fmt_lib():
    L = lib()
    if not getattr(L, "_fmt_ready", False):
        vp, i32, u32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint32
        L.orc_pjw_hash.restype = i32
        L.orc_pjw_hash.argtypes = [vp, ctypes.c_size_t, ctypes.c_int]
        L.orc_base64_encode.restype = ctypes.c_int
        L.orc_base64_encode.argtypes = [vp, ctypes.c_int, vp]
        L.orc_base64_decode.restype = ctypes.c_int
        L.orc_base64_decode.argtypes = [vp, ctypes.c_int, vp]
        L.orc_file_id.restype = None
        L.orc_file_id.argtypes = [u32, i32, ctypes.c_int64, u32, u32, ctypes.c_int, ctypes.c_int,
                                  vp, vp]
        L.orc_parse_file_id.restype = None
        L.orc_parse_file_id.argtypes = [vp, vp, vp, vp, vp]
        L.orc_trunk_pack.restype = None
        L.orc_trunk_pack.argtypes = [ctypes.c_uint8, i32, i32, u32, i32, vp, vp]
        L.orc_fdht_route.restype = None
        L.orc_fdht_route.argtypes = [ctypes.c_char_p, ctypes.c_int, vp, u32, u32, ctypes.c_int,
                                     vp, vp, vp]
        L.orc_fdht_route_key.restype = None
        L.orc_fdht_route_key.argtypes = [ctypes.c_char_p, ctypes.c_int, vp, ctypes.c_int, u32, u32,
                                         ctypes.c_int, vp, vp, vp]
        L._fmt_ready = True
    return L


def pjw_hash(data: bytes, variant: int = VARIANT_SIGNED) -> int:
    return _fmt_lib().orc_pjw_hash(data, len(data), variant)


def base64_encode(data: bytes) -> bytes:
    out = ctypes.create_string_buffer(4 * len(data) // 3 + 4)
    n = _fmt_lib().orc_base64_encode(data, len(data), out)
    return out.raw[:n]


def base64_decode(text: bytes) -> bytes:
    out = ctypes.create_string_buffer(len(text))
    n = _fmt_lib().orc_base64_decode(text, len(text), out)
    return out.raw[:n]


def file_ids(server_id: int, crc32, file_size, timestamp, rnd, subdir_count: int = 256,
             variant: int = VARIANT_SIGNED):
    """(names uint8[n,27], sub_path uint8[n,2]) for a batch."""
    n = len(crc32)
    names = np.zeros((n, 27), np.uint8)
    sub = np.zeros((n, 2), np.uint8)
    L = _fmt_lib()
    for i in range(n):
        L.orc_file_id(server_id, int(timestamp[i]), int(file_size[i]), int(crc32[i]),
                      int(rnd[i]), subdir_count, variant, names[i].ctypes.data,
                      sub[i].ctypes.data)
    return names, sub


def parse_file_ids(names):
    """(server_id u32, timestamp i32, file_size i64, crc32 u32) arrays."""
    names = np.ascontiguousarray(names, np.uint8).reshape(-1, 27)
    n = names.shape[0]
    sid, ts = np.zeros(n, np.uint32), np.zeros(n, np.int32)
    sz, crc = np.zeros(n, np.int64), np.zeros(n, np.uint32)
    L = _fmt_lib()
    for i in range(n):
        L.orc_parse_file_id(names[i].ctypes.data, sid[i:].ctypes.data, ts[i:].ctypes.data,
                            sz[i:].ctypes.data, crc[i:].ctypes.data)
    return sid, ts, sz, crc


def trunk_pack(file_type, alloc_size, file_size, crc32, mtime, ext):
    """uint8[n,24] trunk headers."""
    n = len(crc32)
    ext = np.ascontiguousarray(ext, np.uint8).reshape(n, 7)
    out = np.zeros((n, 24), np.uint8)
    L = _fmt_lib()
    for i in range(n):
        L.orc_trunk_pack(int(file_type[i]), int(alloc_size[i]), int(file_size[i]),
                         int(crc32[i]), int(mtime[i]), ext[i].ctypes.data, out[i].ctypes.data)
    return out


def fdht_route(ns: bytes, sig, group_count: int, servers_per_group,
               variant: int = VARIANT_SIGNED):
    """(key_hash i32, group u32, server u32) per signature."""
    sig = np.ascontiguousarray(sig, np.uint8).reshape(-1, 24)
    n = sig.shape[0]
    kh, grp, srv = np.zeros(n, np.int32), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    L = _fmt_lib()
    for i in range(n):
        g = ctypes.c_uint32()
        L.orc_fdht_route(ns, len(ns), sig[i].ctypes.data, group_count, 1, variant,
                         kh[i:].ctypes.data, ctypes.byref(g), srv[i:].ctypes.data)
        grp[i] = g.value
        L.orc_fdht_route(ns, len(ns), sig[i].ctypes.data, group_count,
                         int(servers_per_group[g.value]), variant, kh[i:].ctypes.data,
                         grp[i:].ctypes.data, srv[i:].ctypes.data)
    return kh, grp, srv


def fdht_route_keys(ns: bytes, keys, lens, group_count: int, servers_per_group,
                    variant: int = VARIANT_SIGNED):
    """(key_hash i32, group u32, server u32) for obj ids keys[i, :lens[i]]."""
    keys = np.ascontiguousarray(keys, np.uint8)
    n = keys.shape[0]
    kh, grp, srv = np.zeros(n, np.int32), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    L = _fmt_lib()
    for i in range(n):
        g = ctypes.c_uint32()
        row = np.ascontiguousarray(keys[i])
        L.orc_fdht_route_key(ns, len(ns), row.ctypes.data, int(lens[i]), group_count, 1, variant,
                             kh[i:].ctypes.data, ctypes.byref(g), srv[i:].ctypes.data)
        grp[i] = g.value
        L.orc_fdht_route_key(ns, len(ns), row.ctypes.data, int(lens[i]), group_count,
                             int(servers_per_group[g.value]), variant, kh[i:].ctypes.data,
                             grp[i:].ctypes.data, srv[i:].ctypes.data)
    return kh, grp, srv
