"""Device-resident batches of objects (the GPU hot path) on torch tensors.

torch supplies device memory and streams only; the arithmetic is libhbec's
HIP kernels, called through the C ABI (``hbec_encode_batch`` /
``hbec_reconstruct_batch``).  Layout of a batch of n one-stripe objects with
shard length S (the ecSplit layout, objectserver/ecutils.go:55-58):

    objs   : uint8 [n, k*S]  — object o's data shard j = objs[o, j*S:(j+1)*S]
    parity : uint8 [n, m*S]  — object o's parity shard r = parity[o, r*S:(r+1)*S]

Shards are never copied: the kernels read the data shards in place.
"""
from __future__ import annotations

import ctypes as C

from . import _native as N
from .reedsolomon import Encoder, check

HBEC_SEED = 0x48424543


def _stream_ptr(stream):
    import torch

    if stream is None:
        stream = torch.cuda.current_stream()
    return C.c_void_p(stream.cuda_stream)


def shard_views(t, n_shards: int, shard_len: int):
    """Views of the n_shards consecutive shards stored in each row of a 2-D tensor."""
    if t.dim() != 2 or t.stride(1) != 1:
        raise ValueError("expected a 2-D row-contiguous tensor")
    if t.shape[1] < n_shards * shard_len:
        raise ValueError("tensor rows shorter than n_shards * shard_len")
    base = t.data_ptr()
    row = t.stride(0) * t.element_size()
    return [(base + i * shard_len, row) for i in range(n_shards)]


def _views(pairs):
    arr = (N.View * len(pairs))()
    for i, (b, s) in enumerate(pairs):
        arr[i].base = b
        arr[i].obj_stride = s
    return arr


def encode_views(enc: Encoder, views, n_objects: int, shard_len: int, stream=None) -> None:
    v = _views(views)
    check(N.lib().hbec_encode_batch(enc.handle, v, int(n_objects), int(shard_len), _stream_ptr(stream)))


def reconstruct_views(enc: Encoder, views, present, n_objects: int, shard_len: int, data_only: bool = False,
                      stream=None) -> None:
    v = _views(views)
    p = (C.c_uint8 * len(present))(*[1 if x else 0 for x in present])
    check(N.lib().hbec_reconstruct_batch(enc.handle, v, p, int(n_objects), int(shard_len), int(data_only),
                                         _stream_ptr(stream)))


def reconstruct_views_mixed(enc: Encoder, views, present, n_objects: int, shard_len: int, data_only: bool = False,
                            stream=None) -> None:
    """reconstruct_views with an erasure pattern per object: ``present`` is an
    [n_objects, k+m] array, row o the mask of object o (non-zero = shard read).
    Equal rows share one pattern (hbec_reconstruct_batch_mixed)."""
    import numpy as np

    v = _views(views)
    p = np.asarray(present) != 0
    if p.ndim != 2 or p.shape[0] != int(n_objects) or p.shape[1] != len(views):
        raise ValueError("present must be [n_objects, k+m]")
    patterns, pattern_of = np.unique(p.astype(np.uint8), axis=0, return_inverse=True)
    patterns = np.ascontiguousarray(patterns, dtype=np.uint8)
    pattern_of = np.ascontiguousarray(pattern_of.reshape(-1), dtype=np.uint32)
    check(N.lib().hbec_reconstruct_batch_mixed(
        enc.handle, v, patterns.ctypes.data_as(N._U8P), patterns.shape[0],
        pattern_of.ctypes.data_as(C.POINTER(C.c_uint32)), int(n_objects), int(shard_len), int(data_only),
        _stream_ptr(stream)))


def mixed_tile_bytes(k: int) -> int:
    """Shard bytes per wave tile of the mixed kernel for k data shards
    (kernels.h stripes_u: 4 / k KiB up to k = 4, 1 KiB above)."""
    return 1024 * (4 // k if k <= 4 else 1)


def mixed_stats():
    """Launches since load of hbec_reconstruct_batch_mixed: of the mixed kernel
    (`mixed`), and of the single-pattern path, one per run of equal-pattern
    objects (`runs`)."""
    a, b = C.c_uint64(), C.c_uint64()
    check(N.lib().hbec_mixed_stats(C.byref(a), C.byref(b)))
    return {"mixed": a.value, "runs": b.value}


def mixed_walk_stats():
    """Mixed-kernel launches since load by the walk of their waves
    (hbec_mixed_walk_stats): a contiguous run of the sorted entry list per wave
    (`contiguous`) or grid-stride (`grid_stride`), and the launches whose waves
    took two tiles or more (`looping`)."""
    a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
    check(N.lib().hbec_mixed_walk_stats(C.byref(a), C.byref(b), C.byref(c)))
    return {"contiguous": a.value, "grid_stride": b.value, "looping": c.value}


def set_mixed_chunk_tiles(tiles: int) -> None:
    """Test hook: mixed-kernel launches of at most `tiles` tiles (0 = default)."""
    check(N.lib().hbec_set_mixed_chunk_tiles(int(tiles)))


def verify_views(enc: Encoder, views, n_objects: int, shard_len: int, flags, stream=None) -> None:
    """Set flags[o] = 1 (uint32 CUDA tensor, caller-zeroed) for objects whose parity is wrong."""
    v = _views(views)
    check(N.lib().hbec_verify_batch(enc.handle, v, int(n_objects), int(shard_len), C.c_void_p(flags.data_ptr()),
                                    _stream_ptr(stream)))


def encode_objects(enc: Encoder, objs, parity, shard_len: int, stream=None) -> None:
    """Encode every row of ``objs`` [n, k*S] into ``parity`` [n, m*S]."""
    n = objs.shape[0]
    if parity.shape[0] != n:
        raise ValueError("objs and parity disagree on the batch size")
    views = shard_views(objs, enc.DataShards, shard_len) + shard_views(parity, enc.ParityShards, shard_len)
    encode_views(enc, views, n, shard_len, stream)


def fill_splitmix(t, obj_len: int, base_seed: int = HBEC_SEED, first: int = 0, stream=None) -> None:
    """Fill row o of a 2-D uint8 tensor with synthetic object (first + o)."""
    if t.dim() != 2 or t.stride(1) != 1:
        raise ValueError("expected a 2-D row-contiguous tensor")
    check(N.lib().hbec_fill_splitmix(C.c_void_p(t.data_ptr()), t.shape[0], int(obj_len),
                                     t.stride(0) * t.element_size(), int(base_seed), int(first),
                                     _stream_ptr(stream)))


def apply_views(rows: int, cols: int, coeffs, in_views, out_views, n_objects: int, shard_len: int,
                stream=None) -> None:
    """Generic GF(2^8) matrix apply: out[r] = XOR_c coeffs[r][c] * in[c]."""
    flat = bytes(int(x) for row in coeffs for x in row)
    cbuf = (C.c_uint8 * len(flat)).from_buffer_copy(flat)
    check(N.lib().hbec_apply_batch(int(rows), int(cols), cbuf, _views(in_views), _views(out_views),
                                   int(n_objects), int(shard_len), _stream_ptr(stream)))


class StripePlan:
    """A device-side plan over stripes of mixed shard lengths (hbec_plan_*).
    `stripes` = [(device address, shard_len)], each stripe being k+m shards
    back to back (ecSplit's databuf layout).  Buffers must outlive the plan's
    queued work."""

    def __init__(self, enc: Encoder, stripes=None, objects=None, shards=None, files=None, chunk_size=None):
        """stripes = [(base, shard_len)] (ecSplit databuf layout), or
        objects = [(data, parity, shard_len)] (data and parity in separate
        regions, hbec_plan_objects), or
        shards = [([address] * (k+m), shard_len)]: every shard of an entry named,
        anywhere and at any alignment (hbec_plan_shards), or
        files = [([address] * (k+m), content_length)] with chunk_size: objects
        given as their k+m shard files, as ecSplit writes them; the library cuts
        them into entries, one per stripe (hbec_plan_files), and
        ``object_start`` (numpy uint32, n_objects + 1) says which: object g is
        entries [object_start[g], object_start[g+1]).  It is what hash_files
        takes, and the arguments indexed by entry (present, flags, where) have
        object_start[-1] rows.
        A shards or files plan takes every call of the other plans; encode,
        reconstruct and verify run the kernels of their _mixed forms, which are
        slower than a stripe or object plan's."""
        self.enc = enc
        self._h = C.c_void_p()
        n = enc.DataShards + enc.ParityShards
        if shards is not None or files is not None:
            import numpy as np

            if (shards is not None) == (files is not None) or stripes is not None or objects is not None:
                raise ValueError("give one of stripes, objects, shards, files")
            if files is not None and chunk_size is None:
                raise ValueError("files needs chunk_size")
            entries = shards if shards is not None else files
            ptrs = (C.c_void_p * max(1, len(entries) * n))()
            lens = np.zeros(max(1, len(entries)), np.uint64)
            for i, (addrs, length) in enumerate(entries):
                if len(addrs) != n:
                    raise ValueError("every entry needs k+m addresses")
                for j, a in enumerate(addrs):
                    ptrs[i * n + j] = a
                lens[i] = length
            if shards is not None:
                self._n = len(shards)
                check(N.lib().hbec_plan_shards(enc.handle, ptrs, lens.ctypes.data_as(C.POINTER(C.c_uint64)),
                                               len(shards), C.byref(self._h)))
                return
            objs = (N.FileObject * max(1, len(files)))()
            for i in range(len(files)):
                objs[i].files = C.cast(C.byref(ptrs, i * n * C.sizeof(C.c_void_p)), C.POINTER(C.c_void_p))
                objs[i].content_length = int(lens[i])
            starts = np.zeros(len(files) + 1, np.uint32)
            self._n = 0
            check(N.lib().hbec_plan_files(enc.handle, objs, len(files), int(chunk_size),
                                          starts.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(self._h)))
            self.object_start = starts
            self._n = int(starts[-1])
            # what glue_files cuts the objects by
            self._content_lengths = [int(x) for x in lens[:len(files)]]
            self._chunk_size = int(chunk_size)
            return
        self._n = len(objects) if objects is not None else len(stripes)
        if objects is not None:
            arr = (N.Object * max(1, len(objects)))()
            for i, (d, p, s) in enumerate(objects):
                arr[i].data, arr[i].parity, arr[i].shard_len = d, p, s
            check(N.lib().hbec_plan_objects(enc.handle, arr, len(objects), C.byref(self._h)))
            return
        arr = (N.Stripe * max(1, len(stripes)))()
        for i, (b, s) in enumerate(stripes):
            arr[i].base = b
            arr[i].shard_len = s
        check(N.lib().hbec_plan_stripes(enc.handle, arr, len(stripes), C.byref(self._h)))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and N._lib is not None:
            N._lib.hbec_plan_free(h)
            self._h = None

    def info(self):
        nt, fb, sb = C.c_uint64(), C.c_uint64(), C.c_uint64()
        tb = C.c_int()
        check(N.lib().hbec_plan_info(self._h, C.byref(nt), C.byref(tb), C.byref(fb), C.byref(sb)))
        return {"n_tiles": nt.value, "tile_bytes": tb.value, "n_fallback": fb.value, "shard_bytes": sb.value}

    def encode(self, stream=None):
        check(N.lib().hbec_encode_plan(self.enc.handle, self._h, _stream_ptr(stream)))

    def reconstruct(self, present, data_only=False, stream=None):
        p = (C.c_uint8 * len(present))(*[1 if x else 0 for x in present])
        check(N.lib().hbec_reconstruct_plan(self.enc.handle, self._h, p, int(data_only), _stream_ptr(stream)))

    def reconstruct_mixed(self, present, data_only=False, stream=None):
        """reconstruct with an erasure pattern per stripe / object: ``present``
        is an [n, k+m] array, row i the mask of entry i of the array the plan
        was built from (zero-length entries included; non-zero = shard read).
        Equal rows share one pattern (hbec_reconstruct_plan_mixed)."""
        import numpy as np

        p = np.asarray(present) != 0
        if p.ndim != 2 or p.shape[0] != self._n or p.shape[1] != self.enc.DataShards + self.enc.ParityShards:
            raise ValueError("present must be [n_stripes, k+m]")
        if self._n == 0:
            patterns, pattern_of = p.astype(np.uint8), np.zeros(0, np.uint32)
        else:
            patterns, pattern_of = np.unique(p.astype(np.uint8), axis=0, return_inverse=True)
        patterns = np.ascontiguousarray(patterns, dtype=np.uint8)
        pattern_of = np.ascontiguousarray(pattern_of.reshape(-1), dtype=np.uint32)
        check(N.lib().hbec_reconstruct_plan_mixed(
            self.enc.handle, self._h, patterns.ctypes.data_as(N._U8P), patterns.shape[0],
            pattern_of.ctypes.data_as(C.POINTER(C.c_uint32)), int(data_only), _stream_ptr(stream)))

    def verify(self, flags, stream=None):
        """flags[i] |= 1 (uint32 CUDA tensor of len(stripes), caller-zeroed) for
        every stripe / object i whose stored parity differs from the recomputed
        one (hbec_verify_plan).  Read-only; queued on the stream."""
        import torch

        if flags.dtype != torch.uint32 and flags.dtype != torch.int32:
            raise ValueError("flags must be a 32-bit integer tensor")
        if not flags.is_cuda or not flags.is_contiguous() or flags.numel() < self._n:
            raise ValueError("flags must be a contiguous CUDA tensor with one entry per stripe")
        check(N.lib().hbec_verify_plan(self.enc.handle, self._h, C.c_void_p(flags.data_ptr()), _stream_ptr(stream)))

    def verify_mixed(self, present, flags, stream=None):
        """verify for a plan whose entries are missing different shards:
        ``present`` is an [n, k+m] array as in reconstruct_mixed.  Per entry the
        present shards beyond its first k present are checked against what those
        k imply: flags[i] |= 1 on a mismatch, |= 2 when exactly k are present and
        nothing could be checked (hbec_verify_plan_mixed).  flags as in verify;
        read-only, queued on the stream."""
        import numpy as np
        import torch

        if flags.dtype != torch.uint32 and flags.dtype != torch.int32:
            raise ValueError("flags must be a 32-bit integer tensor")
        if not flags.is_cuda or not flags.is_contiguous() or flags.numel() < self._n:
            raise ValueError("flags must be a contiguous CUDA tensor with one entry per stripe")
        p = np.asarray(present) != 0
        if p.ndim != 2 or p.shape[0] != self._n or p.shape[1] != self.enc.DataShards + self.enc.ParityShards:
            raise ValueError("present must be [n_stripes, k+m]")
        if self._n == 0:
            patterns, pattern_of = p.astype(np.uint8), np.zeros(0, np.uint32)
        else:
            patterns, pattern_of = np.unique(p.astype(np.uint8), axis=0, return_inverse=True)
        patterns = np.ascontiguousarray(patterns, dtype=np.uint8)
        pattern_of = np.ascontiguousarray(pattern_of.reshape(-1), dtype=np.uint32)
        check(N.lib().hbec_verify_plan_mixed(
            self.enc.handle, self._h, patterns.ctypes.data_as(N._U8P), patterns.shape[0],
            pattern_of.ctypes.data_as(C.POINTER(C.c_uint32)), C.c_void_p(flags.data_ptr()), _stream_ptr(stream)))

    def repair_mixed(self, present, flags, data_only=False, stream=None):
        """verify_mixed and reconstruct_mixed in one pass that reads every
        entry's k survivors once: the missing shards of entry i are rebuilt
        from its first k present shards (missing data shards only with
        data_only) and its other present shards are checked against what those
        k imply; flags[i] |= 1 on a mismatch, |= 2 when exactly k are present
        (hbec_repair_plan_mixed).  A flagged entry's shards are rebuilt all the
        same, from survivors that do not agree with the surplus shards: do not
        commit them; locate_mixed(flags=flags) names the shard to leave out
        and heal_mixed repairs the entry again without it.  ``present`` and ``flags`` as in verify_mixed; queued
        on the stream."""
        import numpy as np
        import torch

        if flags.dtype != torch.uint32 and flags.dtype != torch.int32:
            raise ValueError("flags must be a 32-bit integer tensor")
        if not flags.is_cuda or not flags.is_contiguous() or flags.numel() < self._n:
            raise ValueError("flags must be a contiguous CUDA tensor with one entry per stripe")
        p = np.asarray(present) != 0
        if p.ndim != 2 or p.shape[0] != self._n or p.shape[1] != self.enc.DataShards + self.enc.ParityShards:
            raise ValueError("present must be [n_stripes, k+m]")
        if self._n == 0:
            patterns, pattern_of = p.astype(np.uint8), np.zeros(0, np.uint32)
        else:
            patterns, pattern_of = np.unique(p.astype(np.uint8), axis=0, return_inverse=True)
        patterns = np.ascontiguousarray(patterns, dtype=np.uint8)
        pattern_of = np.ascontiguousarray(pattern_of.reshape(-1), dtype=np.uint32)
        check(N.lib().hbec_repair_plan_mixed(
            self.enc.handle, self._h, patterns.ctypes.data_as(N._U8P), patterns.shape[0],
            pattern_of.ctypes.data_as(C.POINTER(C.c_uint32)), int(data_only), C.c_void_p(flags.data_ptr()),
            _stream_ptr(stream)))

    def locate_mixed(self, present, where, flags=None, stream=None):
        """Name the corrupt shard of every inconsistent entry: ``present`` is an
        [n, k+m] array as in verify_mixed (None: every shard present), ``where``
        a caller-zeroed 32-bit CUDA tensor with one word per entry that is ORed
        into: LOC_BAD, LOC_SKIPPED, LOC_NOTHING and, in bits 0..15, the present
        shards that cannot alone explain some inconsistent byte
        (hbec_locate_plan_mixed; decode with locate_decode).  ``flags``: the
        tensor verify_mixed filled under the same masks; only entries with bit 0
        set are read.  None: every entry is examined.  Read-only apart from
        ``where``; queued on the stream."""
        import numpy as np
        import torch

        n = self.enc.DataShards + self.enc.ParityShards
        for name, t in (("where", where), ("flags", flags)):
            if t is None and name == "flags":
                continue
            if t.dtype != torch.uint32 and t.dtype != torch.int32:
                raise ValueError(f"{name} must be a 32-bit integer tensor")
            if not t.is_cuda or not t.is_contiguous() or t.numel() < self._n:
                raise ValueError(f"{name} must be a contiguous CUDA tensor with one entry per stripe")
        if flags is not None and flags.data_ptr() == where.data_ptr() and self._n:
            raise ValueError("where must not alias flags")
        p = np.ones((self._n, n), bool) if present is None else np.asarray(present) != 0
        if p.ndim != 2 or p.shape[0] != self._n or p.shape[1] != n:
            raise ValueError("present must be [n_stripes, k+m]")
        if self._n == 0:
            patterns, pattern_of = p.astype(np.uint8), np.zeros(0, np.uint32)
        else:
            patterns, pattern_of = np.unique(p.astype(np.uint8), axis=0, return_inverse=True)
        patterns = np.ascontiguousarray(patterns, dtype=np.uint8)
        pattern_of = np.ascontiguousarray(pattern_of.reshape(-1), dtype=np.uint32)
        check(N.lib().hbec_locate_plan_mixed(
            self.enc.handle, self._h, patterns.ctypes.data_as(N._U8P), patterns.shape[0],
            pattern_of.ctypes.data_as(C.POINTER(C.c_uint32)),
            None if flags is None else C.c_void_p(flags.data_ptr()), C.c_void_p(where.data_ptr()),
            _stream_ptr(stream)))

    def heal_mixed(self, present, where, flags, stream=None):
        """Act on locate_mixed's answer on this plan, with nothing copied back:
        every entry whose word of ``where`` names one shard is repaired again
        with that shard left out of its mask.  The named shard and the missing
        ones are rewritten from the first k of the others, flags[i] |= HEAL_DONE
        and repair_mixed's bits for that mask (1: a remaining surplus shard still
        disagrees, 2: none left to check).  An inconsistent entry with no single
        shard named (LOC_AMBIGUOUS, LOC_MULTIPLE) gets flags[i] |= HEAL_UNNAMED
        and is not touched; nor is any other entry (hbec_heal_plan_mixed).
        ``present``: the masks locate_mixed was given (None: every shard
        present); ``where``: its words, read only; ``flags`` as in repair_mixed.
        A sweep is repair_mixed, locate_mixed(flags=flags), heal_mixed, queued
        on one stream with no synchronisation."""
        import numpy as np
        import torch

        n = self.enc.DataShards + self.enc.ParityShards
        for name, t in (("where", where), ("flags", flags)):
            if t.dtype != torch.uint32 and t.dtype != torch.int32:
                raise ValueError(f"{name} must be a 32-bit integer tensor")
            if not t.is_cuda or not t.is_contiguous() or t.numel() < self._n:
                raise ValueError(f"{name} must be a contiguous CUDA tensor with one entry per stripe")
        if flags.data_ptr() == where.data_ptr() and self._n:
            raise ValueError("where must not alias flags")
        p = np.ones((self._n, n), bool) if present is None else np.asarray(present) != 0
        if p.ndim != 2 or p.shape[0] != self._n or p.shape[1] != n:
            raise ValueError("present must be [n_stripes, k+m]")
        if self._n == 0:
            patterns, pattern_of = p.astype(np.uint8), np.zeros(0, np.uint32)
        else:
            patterns, pattern_of = np.unique(p.astype(np.uint8), axis=0, return_inverse=True)
        patterns = np.ascontiguousarray(patterns, dtype=np.uint8)
        pattern_of = np.ascontiguousarray(pattern_of.reshape(-1), dtype=np.uint32)
        check(N.lib().hbec_heal_plan_mixed(
            self.enc.handle, self._h, patterns.ctypes.data_as(N._U8P), patterns.shape[0],
            pattern_of.ctypes.data_as(C.POINTER(C.c_uint32)), C.c_void_p(where.data_ptr()),
            C.c_void_p(flags.data_ptr()), _stream_ptr(stream)))

    def hash_mixed(self, select, digests=None, expected=None, bad=None, where=None, filter=None, filter_bits=1,
                   stream=None):
        """The auditor's check on this plan: the ShardHash (raw MD5) of every
        selected shard of every examined entry, compared on the device with the
        stored one (hbec_hash_plan_mixed).  ``select`` is an [n, k+m] array,
        row i the shards of entry i to hash (any number set; None: every shard).
        ``digests`` and ``expected`` are uint8 CUDA tensors of n*(k+m)*16 bytes,
        shard j of entry i at (i*(k+m) + j)*16; at least one is needed, and
        ``expected`` needs ``bad`` and k+m <= 32.  ``bad``, ``where`` and
        ``filter`` are 32-bit CUDA tensors with one word per entry: bad[i] |=
        1 << j for every hashed shard that differs from ``expected``; where[i]
        (needs ``bad``) gets locate_mixed's word naming that shard, for
        locate_decode and heal_mixed under ``select`` as the masks; only entries
        with filter[i] & filter_bits are examined (None: all).  ``bad`` and
        ``where`` are caller-zeroed and only ORed into.  A sweep that heals a
        stripe with one surplus shard is repair_mixed, hash_mixed(present,
        expected=..., bad=..., where=..., filter=flags), heal_mixed, queued on
        one stream with no synchronisation."""
        import numpy as np
        import torch

        n = self.enc.DataShards + self.enc.ParityShards
        for name, t in (("bad", bad), ("where", where), ("filter", filter)):
            if t is None:
                continue
            if t.dtype != torch.uint32 and t.dtype != torch.int32:
                raise ValueError(f"{name} must be a 32-bit integer tensor")
            if not t.is_cuda or not t.is_contiguous() or t.numel() < self._n:
                raise ValueError(f"{name} must be a contiguous CUDA tensor with one entry per stripe")
        for name, t in (("digests", digests), ("expected", expected)):
            if t is None:
                continue
            if t.dtype != torch.uint8 or not t.is_cuda or not t.is_contiguous() or t.numel() < self._n * n * 16:
                raise ValueError(f"{name} must be a contiguous uint8 CUDA tensor of n * (k+m) * 16 bytes")
        p = np.ones((self._n, n), bool) if select is None else np.asarray(select) != 0
        if p.ndim != 2 or p.shape[0] != self._n or p.shape[1] != n:
            raise ValueError("select must be [n_stripes, k+m]")
        if self._n == 0:
            rows, row_of = p.astype(np.uint8), np.zeros(0, np.uint32)
        else:
            rows, row_of = np.unique(p.astype(np.uint8), axis=0, return_inverse=True)
        rows = np.ascontiguousarray(rows, dtype=np.uint8)
        row_of = np.ascontiguousarray(row_of.reshape(-1), dtype=np.uint32)

        def ptr(t):
            return None if t is None else C.c_void_p(t.data_ptr())

        check(N.lib().hbec_hash_plan_mixed(
            self.enc.handle, self._h, rows.ctypes.data_as(N._U8P), rows.shape[0],
            row_of.ctypes.data_as(C.POINTER(C.c_uint32)), ptr(filter), int(filter_bits) & 0xFFFFFFFF,
            ptr(expected), ptr(digests), ptr(bad), ptr(where), _stream_ptr(stream)))


    def hash_files(self, object_start, select=None, digests=None, expected=None, bad=None, where=None, filter=None,
                   filter_bits=1, stream=None):
        """hash_mixed for objects of more than one stripe: the ShardHash of a
        shard FILE, shard j of each of the object's entries back to back, as
        ecSplit writes it (hbec_hash_plan_files).  ``object_start`` has
        n_objects + 1 entries: object g is the plan's entries
        [object_start[g], object_start[g+1]); it starts at 0, never decreases
        and ends at the plan's entry count.  ``select`` is [n_objects, k+m]
        (None: every shard file).  ``digests`` and ``expected`` hold
        n_objects*(k+m)*16 bytes, file j of object g at (g*(k+m) + j)*16, and
        ``bad`` one word per object.  ``where`` and ``filter`` have one word
        per ENTRY: an object is hashed when any of its entries passes the
        filter, and each passing entry gets the word heal_mixed reads.  The
        sweep is repair_mixed(present, flags), hash_files(object_start,
        select, expected=..., bad=..., where=..., filter=flags),
        heal_mixed(present, where, healed) on one stream, ``present`` being the
        object's row of ``select`` repeated for its entries.  Everything else
        as in hash_mixed, which is the quicker call for one-stripe objects."""
        import numpy as np
        import torch

        n = self.enc.DataShards + self.enc.ParityShards
        starts = np.asarray(object_start)
        if starts.ndim != 1 or starts.size < 1 or starts.dtype.kind not in "iu":
            raise ValueError("object_start must be a 1-D integer array of n_objects + 1 entries")
        if starts.size and (starts.min() < 0 or starts.max() > 0xFFFFFFFF):
            raise ValueError("object_start must hold entry indices")
        starts = np.ascontiguousarray(starts, dtype=np.uint32)
        n_obj = starts.size - 1
        for name, t, need, per in (("bad", bad, n_obj, "object"), ("where", where, self._n, "stripe"),
                                   ("filter", filter, self._n, "stripe")):
            if t is None:
                continue
            if t.dtype != torch.uint32 and t.dtype != torch.int32:
                raise ValueError(f"{name} must be a 32-bit integer tensor")
            if not t.is_cuda or not t.is_contiguous() or t.numel() < need:
                raise ValueError(f"{name} must be a contiguous CUDA tensor with one entry per {per}")
        for name, t in (("digests", digests), ("expected", expected)):
            if t is None:
                continue
            if t.dtype != torch.uint8 or not t.is_cuda or not t.is_contiguous() or t.numel() < n_obj * n * 16:
                raise ValueError(f"{name} must be a contiguous uint8 CUDA tensor of n_objects * (k+m) * 16 bytes")
        p = np.ones((n_obj, n), bool) if select is None else np.asarray(select) != 0
        if p.ndim != 2 or p.shape[0] != n_obj or p.shape[1] != n:
            raise ValueError("select must be [n_objects, k+m]")
        if n_obj == 0:
            rows, row_of = p.astype(np.uint8), np.zeros(0, np.uint32)
        else:
            rows, row_of = np.unique(p.astype(np.uint8), axis=0, return_inverse=True)
        rows = np.ascontiguousarray(rows, dtype=np.uint8)
        row_of = np.ascontiguousarray(row_of.reshape(-1), dtype=np.uint32)

        def ptr(t):
            return None if t is None else C.c_void_p(t.data_ptr())

        check(N.lib().hbec_hash_plan_files(
            self.enc.handle, self._h, starts.ctypes.data_as(C.POINTER(C.c_uint32)), n_obj,
            rows.ctypes.data_as(N._U8P), rows.shape[0], row_of.ctypes.data_as(C.POINTER(C.c_uint32)), ptr(filter),
            int(filter_bits) & 0xFFFFFFFF, ptr(expected), ptr(digests), ptr(bad), ptr(where), _stream_ptr(stream)))

    def _patterns(self, present):
        """The distinct rows of an [n, k+m] present array and each entry's row."""
        import numpy as np

        p = np.asarray(present) != 0
        if p.ndim != 2 or p.shape[0] != self._n or p.shape[1] != self.enc.DataShards + self.enc.ParityShards:
            raise ValueError("present must be [n_stripes, k+m]")
        if self._n == 0:
            patterns, pattern_of = p.astype(np.uint8), np.zeros(0, np.uint32)
        else:
            patterns, pattern_of = np.unique(p.astype(np.uint8), axis=0, return_inverse=True)
        return (np.ascontiguousarray(patterns, dtype=np.uint8),
                np.ascontiguousarray(pattern_of.reshape(-1), dtype=np.uint32))

    def glue_mixed(self, present, dsts, lens, stream=None):
        """ecGlue for every entry in one call (hbec_glue_plan_mixed): entry i's
        data shards 0..k-1 back to back, their first lens[i] bytes, written to
        the device address dsts[i] (any alignment).  ``present`` is [n, k+m] as
        in reconstruct_mixed: a present data shard is copied, a missing one is
        what ReconstructData computes from the entry's first k present shards.
        No shard is written; lens[i] = 0 skips the entry, lens[i] <= k * S_i.
        Queued on the stream."""
        import numpy as np

        patterns, pattern_of = self._patterns(present)
        if len(dsts) != self._n or len(lens) != self._n:
            raise ValueError("dsts and lens need one element per entry")
        d = (C.c_void_p * max(1, self._n))(*[int(a) for a in dsts])
        ln = np.zeros(max(1, self._n), np.uint64)
        ln[:self._n] = [int(x) for x in lens]
        check(N.lib().hbec_glue_plan_mixed(
            self.enc.handle, self._h, patterns.ctypes.data_as(N._U8P), patterns.shape[0],
            pattern_of.ctypes.data_as(C.POINTER(C.c_uint32)), d, ln.ctypes.data_as(C.POINTER(C.c_uint64)),
            _stream_ptr(stream)))

    def glue_files(self, present, outs, stream=None):
        """glue_mixed for a ``files=`` plan, object by object
        (hbec_glue_plan_files): object g is written whole, its content length
        in bytes, at the device address outs[g].  ``present`` stays per ENTRY
        ([object_start[-1], k+m]): a file may fail between two stripes."""
        import numpy as np

        if getattr(self, "_content_lengths", None) is None:
            raise ValueError("glue_files needs a plan built from files=")
        patterns, pattern_of = self._patterns(present)
        n_obj = len(self._content_lengths)
        if len(outs) != n_obj:
            raise ValueError("outs needs one address per object")
        d = (C.c_void_p * max(1, n_obj))(*[int(a) for a in outs])
        ln = np.zeros(max(1, n_obj), np.uint64)
        ln[:n_obj] = self._content_lengths
        starts = np.ascontiguousarray(self.object_start, dtype=np.uint32)
        check(N.lib().hbec_glue_plan_files(
            self.enc.handle, self._h, starts.ctypes.data_as(C.POINTER(C.c_uint32)), n_obj,
            ln.ctypes.data_as(C.POINTER(C.c_uint64)), int(self._chunk_size), patterns.ctypes.data_as(N._U8P),
            patterns.shape[0], pattern_of.ctypes.data_as(C.POINTER(C.c_uint32)), d, _stream_ptr(stream)))

    def glue_range(self, present, dsts, starts, lens, stream=None):
        """Any byte range of every entry in one call (hbec_glue_plan_range): with
        D_i entry i's data shards 0..k-1 back to back as in glue_mixed, the
        bytes D_i[starts[i], starts[i] + lens[i]) are written to the device
        address dsts[i] (any alignment), and nothing else.  Tiles of shard
        positions outside the range are not read, and a part of the range that
        touches no missing data shard is copied without decoding.  lens[i] = 0
        skips the entry; starts[i] + lens[i] <= k * S_i.  Queued on the stream."""
        import numpy as np

        patterns, pattern_of = self._patterns(present)
        if len(dsts) != self._n or len(starts) != self._n or len(lens) != self._n:
            raise ValueError("dsts, starts and lens need one element per entry")
        d = (C.c_void_p * max(1, self._n))(*[int(a) for a in dsts])
        st, ln = np.zeros(max(1, self._n), np.uint64), np.zeros(max(1, self._n), np.uint64)
        st[:self._n] = [int(x) for x in starts]
        ln[:self._n] = [int(x) for x in lens]
        check(N.lib().hbec_glue_plan_range(
            self.enc.handle, self._h, patterns.ctypes.data_as(N._U8P), patterns.shape[0],
            pattern_of.ctypes.data_as(C.POINTER(C.c_uint32)), d, st.ctypes.data_as(C.POINTER(C.c_uint64)),
            ln.ctypes.data_as(C.POINTER(C.c_uint64)), _stream_ptr(stream)))

    def glue_range_files(self, present, outs, starts, ends, stream=None):
        """glue_range for a ``files=`` plan, object by object
        (hbec_glue_plan_files_range): object g's bytes [starts[g], ends[g]), in
        object bytes, are written to the device address outs[g].  ``present``
        stays per ENTRY, as in glue_files."""
        import numpy as np

        if getattr(self, "_content_lengths", None) is None:
            raise ValueError("glue_range_files needs a plan built from files=")
        patterns, pattern_of = self._patterns(present)
        n_obj = len(self._content_lengths)
        if len(outs) != n_obj or len(starts) != n_obj or len(ends) != n_obj:
            raise ValueError("outs, starts and ends need one element per object")
        d = (C.c_void_p * max(1, n_obj))(*[int(a) for a in outs])
        ln, st, en = (np.zeros(max(1, n_obj), np.uint64) for _ in range(3))
        ln[:n_obj] = self._content_lengths
        st[:n_obj] = [int(x) for x in starts]
        en[:n_obj] = [int(x) for x in ends]
        object_start = np.ascontiguousarray(self.object_start, dtype=np.uint32)
        check(N.lib().hbec_glue_plan_files_range(
            self.enc.handle, self._h, object_start.ctypes.data_as(C.POINTER(C.c_uint32)), n_obj,
            ln.ctypes.data_as(C.POINTER(C.c_uint64)), int(self._chunk_size), patterns.ctypes.data_as(N._U8P),
            patterns.shape[0], pattern_of.ctypes.data_as(C.POINTER(C.c_uint32)), d,
            st.ctypes.data_as(C.POINTER(C.c_uint64)), en.ctypes.data_as(C.POINTER(C.c_uint64)), _stream_ptr(stream)))

    def _etag_tensors(self, n_slots, per, digests, expected, bad, filter):
        """The shape and dtype checks of etag_mixed / etag_files."""
        import torch

        for name, t, need, what in (("bad", bad, n_slots, per), ("filter", filter, self._n, "stripe")):
            if t is None:
                continue
            if t.dtype != torch.uint32 and t.dtype != torch.int32:
                raise ValueError(f"{name} must be a 32-bit integer tensor")
            if not t.is_cuda or not t.is_contiguous() or t.numel() < need:
                raise ValueError(f"{name} must be a contiguous CUDA tensor with one entry per {what}")
        for name, t in (("digests", digests), ("expected", expected)):
            if t is None:
                continue
            if t.dtype != torch.uint8 or not t.is_cuda or not t.is_contiguous() or t.numel() < n_slots * 16:
                raise ValueError(f"{name} must be a contiguous uint8 CUDA tensor of 16 bytes per {per}")
        if expected is not None and bad is None:
            raise ValueError("expected needs bad")

    def etag_mixed(self, present, lens, digests=None, expected=None, bad=None, filter=None, filter_bits=1,
                   stream=None):
        """The ETag check of every entry in one call (hbec_etag_plan_mixed): the
        raw MD5 of entry i's data shards 0..k-1 back to back, their first
        lens[i] bytes, hashed where they lie.  ``present`` is [n, k+m] as in
        glue_mixed (None: every shard present): a missing data shard with a
        byte below lens[i] is decoded into scratch first and read from there; no
        shard and no object-sized buffer is written.  ``digests`` and
        ``expected`` are uint8 CUDA tensors of n*16 bytes (at least one is
        needed); ``bad`` and ``filter`` are 32-bit CUDA tensors with one word
        per entry: bad[i] |= 1 where the digest differs from ``expected``
        (caller-zeroed, needed with ``expected``), and only entries with
        filter[i] & filter_bits are examined (None: all).  lens[i] = 0 skips the
        entry; lens[i] <= k * S_i.  After a repair, a rebuilt data shard has no
        stored ShardHash; the stored ETag is its check: repair_mixed, then
        etag_mixed(None, lens, expected=etags, bad=bad) on one stream."""
        import numpy as np

        n = self.enc.DataShards + self.enc.ParityShards
        self._etag_tensors(self._n, "stripe", digests, expected, bad, filter)
        patterns, pattern_of = self._patterns(np.ones((self._n, n), bool) if present is None else present)
        if len(lens) != self._n:
            raise ValueError("lens needs one element per entry")
        ln = np.zeros(max(1, self._n), np.uint64)
        ln[:self._n] = [int(x) for x in lens]

        def ptr(t):
            return None if t is None else C.c_void_p(t.data_ptr())

        check(N.lib().hbec_etag_plan_mixed(
            self.enc.handle, self._h, patterns.ctypes.data_as(N._U8P), patterns.shape[0],
            pattern_of.ctypes.data_as(C.POINTER(C.c_uint32)), ln.ctypes.data_as(C.POINTER(C.c_uint64)), ptr(filter),
            int(filter_bits) & 0xFFFFFFFF, ptr(expected), ptr(digests), ptr(bad), _stream_ptr(stream)))

    def etag_files(self, present, digests=None, expected=None, bad=None, filter=None, filter_bits=1, stream=None):
        """etag_mixed for a ``files=`` plan, object by object
        (hbec_etag_plan_files): the ETag of object g, the MD5 of the bytes
        glue_files would write for it, its stripes hashed as one stream.
        ``digests`` and ``expected`` hold n_objects*16 bytes and ``bad`` one
        word per object; ``present`` and ``filter`` stay per ENTRY, and an
        object is hashed when any of its entries passes the filter.  The
        lengths are the plan's; an object with no byte is left untouched."""
        import numpy as np

        if getattr(self, "_content_lengths", None) is None:
            raise ValueError("etag_files needs a plan built from files=")
        n = self.enc.DataShards + self.enc.ParityShards
        n_obj = len(self._content_lengths)
        self._etag_tensors(n_obj, "object", digests, expected, bad, filter)
        patterns, pattern_of = self._patterns(np.ones((self._n, n), bool) if present is None else present)
        ln = np.zeros(max(1, n_obj), np.uint64)
        ln[:n_obj] = self._content_lengths
        starts = np.ascontiguousarray(self.object_start, dtype=np.uint32)

        def ptr(t):
            return None if t is None else C.c_void_p(t.data_ptr())

        check(N.lib().hbec_etag_plan_files(
            self.enc.handle, self._h, starts.ctypes.data_as(C.POINTER(C.c_uint32)), n_obj,
            ln.ctypes.data_as(C.POINTER(C.c_uint64)), int(self._chunk_size), patterns.ctypes.data_as(N._U8P),
            patterns.shape[0], pattern_of.ctypes.data_as(C.POINTER(C.c_uint32)), ptr(filter),
            int(filter_bits) & 0xFFFFFFFF, ptr(expected), ptr(digests), ptr(bad), _stream_ptr(stream)))

    def split(self, srcs, lens, stream=None):
        """ecSplit for every entry in one call (hbec_split_plan), the inverse
        of glue_mixed: the lens[i] bytes at the device address srcs[i] (any
        alignment) are cut into entry i's k data shards, zero-padded as ecSplit
        pads its last stripe, and its m parity shards are coded from them.  All
        k+m shards are written whole; the source is read once.  lens[i] = 0
        skips the entry; otherwise ceil(lens[i] / k) must be the entry's shard
        length.  Queued on the stream."""
        import numpy as np

        if len(srcs) != self._n or len(lens) != self._n:
            raise ValueError("srcs and lens need one element per entry")
        d = (C.c_void_p * max(1, self._n))(*[int(a) for a in srcs])
        ln = np.zeros(max(1, self._n), np.uint64)
        ln[:self._n] = [int(x) for x in lens]
        check(N.lib().hbec_split_plan(self.enc.handle, self._h, d, ln.ctypes.data_as(C.POINTER(C.c_uint64)),
                                      _stream_ptr(stream)))

    def split_files(self, srcs, stream=None):
        """split for a ``files=`` plan, object by object (hbec_split_plan_files):
        object g, its content length in bytes at the device address srcs[g],
        is written as its k+m shard files, which is ecSplit for the batch."""
        import numpy as np

        if getattr(self, "_content_lengths", None) is None:
            raise ValueError("split_files needs a plan built from files=")
        n_obj = len(self._content_lengths)
        if len(srcs) != n_obj:
            raise ValueError("srcs needs one address per object")
        d = (C.c_void_p * max(1, n_obj))(*[int(a) for a in srcs])
        ln = np.zeros(max(1, n_obj), np.uint64)
        ln[:n_obj] = self._content_lengths
        starts = np.ascontiguousarray(self.object_start, dtype=np.uint32)
        check(N.lib().hbec_split_plan_files(
            self.enc.handle, self._h, starts.ctypes.data_as(C.POINTER(C.c_uint32)), n_obj,
            ln.ctypes.data_as(C.POINTER(C.c_uint64)), int(self._chunk_size), d, _stream_ptr(stream)))


def glue_plan_stats():
    """Since load, for StripePlan.glue_mixed / glue_files: launches of the glue
    kernel (`kernel_launches`) and, on the per-entry route, device-to-device
    copies and single-pattern applies (`per_stripe_calls`)."""
    a, b = C.c_uint64(), C.c_uint64()
    check(N.lib().hbec_glue_plan_stats(C.byref(a), C.byref(b)))
    return {"kernel_launches": a.value, "per_stripe_calls": b.value}


def glue_plan_tile_bytes() -> int:
    """Shard bytes per wave tile of the glue kernel."""
    return int(N.lib().hbec_glue_plan_tile_bytes())


def set_glue_plan_chunk_tiles(tiles: int) -> None:
    """Test hook: glue kernel launches of at most `tiles` tiles (0 = default)."""
    check(N.lib().hbec_set_glue_plan_chunk_tiles(int(tiles)))


def glue_range_stats():
    """Since load, for StripePlan.glue_range / glue_range_files: launches of the
    range kernel (`kernel_launches`) and, on the per-entry route,
    device-to-device copies and single-pattern applies (`per_stripe_calls`)."""
    a, b = C.c_uint64(), C.c_uint64()
    check(N.lib().hbec_glue_range_stats(C.byref(a), C.byref(b)))
    return {"kernel_launches": a.value, "per_stripe_calls": b.value}


def glue_range_tile_bytes() -> int:
    """Shard bytes per wave tile of the range kernel."""
    return int(N.lib().hbec_glue_range_tile_bytes())


def set_glue_range_chunk_tiles(tiles: int) -> None:
    """Test hook: range kernel launches of at most `tiles` tiles (0 = default)."""
    check(N.lib().hbec_set_glue_range_chunk_tiles(int(tiles)))


def etag_plan_stats():
    """Since load, for StripePlan.etag_mixed / etag_files: launches of the chain
    kernel md5_etag (`kernel_launches`), chains listed, one per object with a
    byte in it (`chains`), the segments those chains walk as the host lists
    them (`segments`), and the entries of which any missing data byte was
    decoded beforehand (`decoded_entries`)."""
    a, b, c, d = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
    check(N.lib().hbec_etag_plan_stats(C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
    return {"kernel_launches": a.value, "chains": b.value, "segments": c.value, "decoded_entries": d.value}


def split_plan_stats():
    """Since load, for StripePlan.split / split_files: launches of the split
    kernel (`kernel_launches`) and, on the per-entry route, device-to-device
    copies, memsets and applies (`per_stripe_calls`)."""
    a, b = C.c_uint64(), C.c_uint64()
    check(N.lib().hbec_split_plan_stats(C.byref(a), C.byref(b)))
    return {"kernel_launches": a.value, "per_stripe_calls": b.value}


def split_plan_tile_bytes() -> int:
    """Shard bytes per wave tile of the split kernel."""
    return int(N.lib().hbec_split_plan_tile_bytes())


def set_split_plan_chunk_tiles(tiles: int) -> None:
    """Test hook: split kernel launches of at most `tiles` tiles (0 = default)."""
    check(N.lib().hbec_set_split_plan_chunk_tiles(int(tiles)))


def hash_files_stats():
    """Since load, for StripePlan.hash_files: launches of its kernels, md5_files
    and (with ``where``) hash_files_where (`kernel_launches`), chains listed,
    one per selected shard file of an object with a byte in it (`chains`), and
    the non-empty entries those chains walk, once per chain (`segments`)."""
    a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
    check(N.lib().hbec_hash_files_stats(C.byref(a), C.byref(b), C.byref(c)))
    return {"kernel_launches": a.value, "chains": b.value, "segments": c.value}


def hash_plan_stats():
    """Since load, for StripePlan.hash_mixed: launches of its kernels, md5_plan
    and (with ``where``) hash_where (`kernel_launches`), and chains listed, one
    per selected shard of a non-empty entry (`chains`)."""
    a, b = C.c_uint64(), C.c_uint64()
    check(N.lib().hbec_hash_plan_stats(C.byref(a), C.byref(b)))
    return {"kernel_launches": a.value, "chains": b.value}


def locate_decode(k: int, m: int, present, where_array):
    """The shard every word of ``where_array`` names (hbec_locate_decode; host
    only): an int array of shard indices, or LOC_CLEAN, LOC_AMBIGUOUS,
    LOC_MULTIPLE, LOC_UNCHECKED.  ``present``: [n, k+m] masks as given to
    locate_mixed, one mask for all, or None (every shard present)."""
    import numpy as np

    w = np.asarray(where_array).reshape(-1).astype(np.int64) & 0xFFFFFFFF
    p = np.ones((1, k + m), np.uint8) if present is None else np.asarray(present) != 0
    p = np.ascontiguousarray(np.atleast_2d(p), dtype=np.uint8)
    if p.shape[1] != k + m or p.shape[0] not in (1, w.size):
        raise ValueError("present must be [n, k+m] or one mask of k+m")
    fn = N.lib().hbec_locate_decode
    out = np.empty(w.size, np.int64)
    for i in range(w.size):
        row = p[i if p.shape[0] > 1 else 0]
        out[i] = fn(int(k), int(m), row.ctypes.data_as(N._U8P), int(w[i]))
        if out[i] == N.ERR_INVALID_ARG:
            raise ValueError("bad (k, m)")
    return out


def locate_plan_stats():
    """Since load, for StripePlan.locate_mixed: launches of the locate kernel
    (`kernel_launches`) and entries of a shape it does not take, marked
    LOC_SKIPPED (`skipped_entries`)."""
    a, b = C.c_uint64(), C.c_uint64()
    check(N.lib().hbec_locate_plan_stats(C.byref(a), C.byref(b)))
    return {"kernel_launches": a.value, "skipped_entries": b.value}


def locate_plan_tile_bytes() -> int:
    """Shard bytes per wave tile of the locate kernel."""
    return int(N.lib().hbec_locate_plan_tile_bytes())


def set_locate_plan_chunk_tiles(tiles: int) -> None:
    """Test hook: locate kernel launches of at most `tiles` tiles (0 = default)."""
    check(N.lib().hbec_set_locate_plan_chunk_tiles(int(tiles)))


def repair_plan_stats():
    """Since load, for StripePlan.repair_mixed: launches of the repair kernel
    (`kernel_launches`) and entries repaired one at a time for the shapes that
    kernel does not take (`per_stripe_calls`)."""
    a, b = C.c_uint64(), C.c_uint64()
    check(N.lib().hbec_repair_plan_stats(C.byref(a), C.byref(b)))
    return {"kernel_launches": a.value, "per_stripe_calls": b.value}


def repair_plan_tile_bytes() -> int:
    """Shard bytes per wave tile of the repair kernel."""
    return int(N.lib().hbec_repair_plan_tile_bytes())


def set_repair_plan_chunk_tiles(tiles: int) -> None:
    """Test hook: repair kernel launches of at most `tiles` tiles (0 = default)."""
    check(N.lib().hbec_set_repair_plan_chunk_tiles(int(tiles)))


def heal_plan_stats():
    """Since load, for StripePlan.heal_mixed: launches of the heal kernel
    (`kernel_launches`) and entries of a shape it does not take, left alone
    (`skipped_entries`)."""
    a, b = C.c_uint64(), C.c_uint64()
    check(N.lib().hbec_heal_plan_stats(C.byref(a), C.byref(b)))
    return {"kernel_launches": a.value, "skipped_entries": b.value}


def heal_plan_tile_bytes() -> int:
    """Shard bytes per wave tile of the heal kernel."""
    return int(N.lib().hbec_heal_plan_tile_bytes())


def set_heal_plan_chunk_tiles(tiles: int) -> None:
    """Test hook: heal kernel launches of at most `tiles` tiles (0 = default)."""
    check(N.lib().hbec_set_heal_plan_chunk_tiles(int(tiles)))


def verify_plan_stats():
    """Since load: launches of the plan Verify kernels (`plan_launches`) and
    verify calls made one stripe at a time for the shapes those kernels do not
    take (`per_stripe_calls`)."""
    a, b = C.c_uint64(), C.c_uint64()
    check(N.lib().hbec_verify_plan_stats(C.byref(a), C.byref(b)))
    return {"plan_launches": a.value, "per_stripe_calls": b.value}


def verify_route_stats():
    """verify_views calls since load by the branch that answered them
    (hbec_verify_route_stats): packed, pipe, records (16-B-aligned shapes sent
    to the record kernels; counted under odd too), odd, wide, unaligned, scratch."""
    r = N.VerifyRoutes()
    check(N.lib().hbec_verify_route_stats(C.byref(r)))
    return {n: getattr(r, n) for n, _ in N.VerifyRoutes._fields_}


def apply_route_stats():
    """apply_views passes since load by the branch that coded them
    (hbec_apply_route_stats): packed, vec, odd (the gf_odd families, 16-B-aligned
    shapes sent to the record kernels included), unaligned, wide (one per call)."""
    r = N.ApplyRoutes()
    check(N.lib().hbec_apply_route_stats(C.byref(r)))
    return {n: getattr(r, n) for n, _ in N.ApplyRoutes._fields_}


def verify_plan_tile_bytes(k: int) -> int:
    """Shard bytes per wave tile of the any-alignment plan Verify kernel."""
    return int(N.lib().hbec_verify_plan_tile_bytes(int(k)))


def mixed_plan_stats():
    """Since load, for StripePlan.reconstruct_mixed: launches of the mixed plan
    kernel (`kernel_launches`) and single-pattern applies made one stripe at a
    time for the shapes that kernel does not take (`per_stripe_calls`)."""
    a, b = C.c_uint64(), C.c_uint64()
    check(N.lib().hbec_mixed_plan_stats(C.byref(a), C.byref(b)))
    return {"kernel_launches": a.value, "per_stripe_calls": b.value}


def mixed_plan_tile_bytes() -> int:
    """Shard bytes per wave tile of the mixed plan kernel."""
    return int(N.lib().hbec_mixed_plan_tile_bytes())


def set_mixed_plan_chunk_tiles(tiles: int) -> None:
    """Test hook: mixed plan kernel launches of at most `tiles` tiles (0 = default)."""
    check(N.lib().hbec_set_mixed_plan_chunk_tiles(int(tiles)))


def verify_mixed_plan_stats():
    """Since load, for StripePlan.verify_mixed: launches of the mixed plan Verify
    kernel (`kernel_launches`) and stripes verified one at a time for the shapes
    that kernel does not take (`per_stripe_calls`)."""
    a, b = C.c_uint64(), C.c_uint64()
    check(N.lib().hbec_verify_mixed_plan_stats(C.byref(a), C.byref(b)))
    return {"kernel_launches": a.value, "per_stripe_calls": b.value}


def verify_mixed_plan_tile_bytes() -> int:
    """Shard bytes per wave tile of the mixed plan Verify kernel."""
    return int(N.lib().hbec_verify_mixed_plan_tile_bytes())


def set_verify_mixed_plan_chunk_tiles(tiles: int) -> None:
    """Test hook: mixed plan Verify kernel launches of at most `tiles` tiles (0 = default)."""
    check(N.lib().hbec_set_verify_mixed_plan_chunk_tiles(int(tiles)))


KERNEL_KINDS = {0: "unrolled", 1: "pipelined", 2: "streaming", 3: "packed", 4: "records"}


def kernel_info(k: int, r: int, shard_len: int):
    tb, kind, bpc = C.c_int(), C.c_int(), C.c_int()
    check(N.lib().hbec_kernel_info(k, r, int(shard_len), C.byref(tb), C.byref(kind), C.byref(bpc)))
    return {"tile_bytes": tb.value, "kind": KERNEL_KINDS[kind.value], "blocks_per_cu": bpc.value}


def odd_path_stats():
    """Launches since load of the odd-shard main kernels, by family:
    bit-plane (compiled encode XOR networks), table-multiply records, strided;
    and the guard bands: separate edge-kernel launches (`edges`) and main
    launches that coded their own (`fused`)."""
    b, r, s = C.c_uint64(), C.c_uint64(), C.c_uint64()
    check(N.lib().hbec_odd_path_stats(C.byref(b), C.byref(r), C.byref(s)))
    e, f = C.c_uint64(), C.c_uint64()
    check(N.lib().hbec_odd_edge_stats(C.byref(e), C.byref(f)))
    return {"bitplane": b.value, "records": r.value, "strided": s.value, "edges": e.value, "fused": f.value}


def odd_record_cache(clear: bool = False):
    """(cached view sets, calls that reused one) of the strided record
    passes' record cache; clear=True drops it (test hook, device synchronised)."""
    e, h = C.c_uint64(), C.c_uint64()
    check(N.lib().hbec_odd_record_cache(1 if clear else 0, C.byref(e), C.byref(h)))
    return e.value, h.value


def set_odd_chunk_tiles(tiles: int) -> None:
    """Test hook: odd-shard strided launches of at most `tiles` tiles (0 = default)."""
    N.lib().hbec_set_odd_chunk_tiles(int(tiles))


def set_vec_chunk_tiles(tiles: int) -> None:
    """Test hook: aligned strided launches, packed ones included, of at most `tiles` tiles (0 = default)."""
    check(N.lib().hbec_set_vec_chunk_tiles(int(tiles)))


def set_vec_grid_cap(blocks: int) -> None:
    """Test hook: at most `blocks` blocks per aligned strided launch, packed ones included (0 = no cap)."""
    check(N.lib().hbec_set_vec_grid_cap(int(blocks)))


def vec_launch_config() -> tuple[int, int]:
    """(tiles per launch, grid cap) of the aligned strided kernels now in force."""
    t, g = C.c_uint64(), C.c_int()
    check(N.lib().hbec_vec_launch_config(C.byref(t), C.byref(g)))
    return t.value, g.value


def vec_kernel_stats():
    """Launches since load of the aligned strided apply kernels, by the kernel
    launched (hbec_vec_kernel_stats): packed, pipe2, pipe, vec, stream."""
    v = [C.c_uint64() for _ in range(5)]
    check(N.lib().hbec_vec_kernel_stats(*[C.byref(x) for x in v]))
    return dict(zip(("packed", "pipe2", "pipe", "vec", "stream"), (x.value for x in v)))


STRIPES_VARIANTS = ("plain", "split", "accumulate", "mirror", "mirror_accumulate")


def stripes_kernel_stats():
    """Launches since load of the tiled stripes kernel gf_apply_stripes, by
    variant (hbec_stripes_kernel_stats)."""
    v = [C.c_uint64() for _ in STRIPES_VARIANTS]
    check(N.lib().hbec_stripes_kernel_stats(*[C.byref(x) for x in v]))
    return dict(zip(STRIPES_VARIANTS, (x.value for x in v)))


def set_stripes_grid_cap(blocks: int) -> None:
    """Test hook: at most `blocks` blocks per gf_apply_stripes launch (0 = no cap)."""
    check(N.lib().hbec_set_stripes_grid_cap(int(blocks)))


def host_run_stats():
    """How the host calls cut their work since load (hbec_host_run_stats):
    staging chunks, column pieces, zero-copy record slots, hash arena flushes."""
    names = ("ring_chunks", "ring_pieces", "zc_record_slots", "arena_flushes")
    v = [C.c_uint64() for _ in names]
    check(N.lib().hbec_host_run_stats(*[C.byref(x) for x in v]))
    return dict(zip(names, (x.value for x in v)))


def pipe2_store_depth(k: int, r: int) -> tuple[int, bool]:
    """(store depth, run walk) of the pipelined kernel of a k x r pass."""
    d, run = C.c_int(), C.c_int()
    check(N.lib().hbec_pipe2_store_depth(k, r, C.byref(d), C.byref(run)))
    return d.value, bool(run.value)


def set_force_stream(on: bool) -> None:
    N.lib().hbec_set_force_stream(1 if on else 0)
