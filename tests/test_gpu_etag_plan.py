"""hbec_etag_plan_mixed and hbec_etag_plan_files on the device: the MD5 of the
object bytes of a plan's entries and objects, hashed where they lie in the data
shards, degraded or not, on all four kinds of plan.

Nothing expected comes from the product.  Every digest is hashlib.md5 of bytes
put together in numpy: an entry's D is oracle.object_bytes, all k S of it, so
whatever lies beyond lens is non-zero garbage the parity (coracle.apply of the
coding matrix) agrees with; a files object is oracle.ec_split's shard files.
The shards a mask calls missing hold 0xD7 in device memory, so a digest can only
be right through the decode.  After each call the whole arena, every shard and
the gaps between them, is compared with its copy: the call is read-only.
digests and bad are prefilled (0xA5, 0x100), so untouched slots show."""
import hashlib

import numpy as np
import pytest
import torch

import test_etag_host as EH
from hummingbird_amd import batch as B
from hummingbird_amd import reedsolomon as RS
from oracle import coracle as CO
from oracle import oracle as O

pytestmark = pytest.mark.gpu

GARBAGE, GAP, DIG, BAD0 = 0xD7, 0x3C, 0xA5, 0x100
_WORDS = {}


class Word:
    """One codeword: D (k S bytes of object_bytes), its k+m shards, and hashlib's MD5 of every prefix asked for."""

    def __init__(self, k, m, S, seed):
        self.k, self.m, self.S = k, m, S
        self.D = np.asarray(O.object_bytes(seed, k * S), np.uint8).copy() if S else np.zeros(0, np.uint8)
        data = [self.D[j * S:(j + 1) * S] for j in range(k)]
        par = CO.apply(CO.build_matrix(k, m)[k:], data) if S and m else [np.zeros(0, np.uint8)] * m
        self.shards = data + list(par)
        self._md5 = {}

    def md5(self, ln):
        if ln not in self._md5:
            self._md5[ln] = hashlib.md5(self.D[:ln].tobytes()).digest()
        return self._md5[ln]


def word(k, m, S, seed=None):
    """The shared codeword of a shape: computed once, never changed."""
    key = (k, m, S, seed)
    if key not in _WORDS:
        _WORDS[key] = Word(k, m, S, 7000 + 131 * k + S if seed is None else seed)
    return _WORDS[key]


class Arena:
    """Codewords laid out in one device buffer, for one kind of plan.  put()
    returns the plan entry of a codeword: the shards a mask calls missing are
    GARBAGE, `flip` = (shard, position, bit) turns one bit of a shard."""

    def __init__(self, kind):
        self.kind, self.img, self.spec = kind, bytearray(b"\x3c" * 64), []

    def _at(self, blob, residue):
        while len(self.img) % 4 != residue % 4:
            self.img.append(GAP)
        off = len(self.img)
        self.img += bytes(blob)
        self.img += bytes([GAP] * 5)
        return off

    def put(self, w, mask, residue=0, flip=None):
        k, m, S = w.k, w.m, w.S
        sh = [np.full(S, GARBAGE, np.uint8) if not mask[j] else w.shards[j].copy() for j in range(k + m)]
        if flip is not None:
            sh[flip[0]][flip[1]] ^= 1 << flip[2]
        if self.kind == "stripes":
            self.spec.append(("s", self._at(np.concatenate(sh) if S else b"", residue), S))
        elif self.kind == "objects":
            d = self._at(np.concatenate(sh[:k]) if S else b"", residue)
            p = self._at(np.concatenate(sh[k:]) if S and m else b"", residue + 1)
            self.spec.append(("o", d, p, S))
        else:  # every shard at its own address and residue, in scrambled order
            offs = [0] * (k + m)
            for j in sorted(range(k + m), key=lambda j: (j * 5 + 2) % (k + m)):
                offs[j] = self._at(sh[j], residue + j)
            self.spec.append(("r", offs, S))
        return len(self.spec) - 1

    def build(self, enc):
        self.dev = torch.from_numpy(np.frombuffer(bytes(self.img), np.uint8).copy()).cuda()
        self.copy = self.dev.clone()
        base = self.dev.data_ptr()
        assert base % 4 == 0
        if self.kind == "stripes":
            self.plan = B.StripePlan(enc, stripes=[(base + o if S else 0, S) for _, o, S in self.spec])
        elif self.kind == "objects":
            self.plan = B.StripePlan(enc, objects=[(base + d if S else 0, base + p if S else 0, S)
                                                   for _, d, p, S in self.spec])
        else:
            self.plan = B.StripePlan(enc, shards=[([base + o if S else 0 for o in offs], S)
                                                  for _, offs, S in self.spec])
        return self.plan

    def unchanged(self):
        return torch.equal(self.dev, self.copy)


def slots(n):
    """Prefilled digests and bad for n slots."""
    return (torch.full((max(1, n) * 16,), DIG, dtype=torch.uint8, device="cuda"),
            torch.full((max(1, n),), BAD0, dtype=torch.int32, device="cuda"))


def expected_of(md5s):
    """A device tensor of the given digests (None: 16 bytes that match nothing)."""
    raw = b"".join(d if d is not None else b"\x11" * 16 for d in md5s) or b"\0" * 16
    return torch.from_numpy(np.frombuffer(raw, np.uint8).copy()).cuda()


def check_slots(dig, bad, md5s, wrong=()):
    """Slot i holds md5s[i] and bad BAD0 (BAD0 | 1 for i in wrong); md5s[i] None: both untouched."""
    torch.cuda.synchronize()
    got = dig.cpu().numpy().tobytes()
    b = bad.cpu().numpy()
    for i, d in enumerate(md5s):
        want = bytes([DIG] * 16) if d is None else d
        assert got[16 * i:16 * i + 16] == want, (i, got[16 * i:16 * i + 16].hex(), want.hex())
        assert b[i] == (BAD0 | 1 if i in wrong else BAD0), (i, hex(b[i]))


def model_decoded(k, S, ln, mask):
    return any(not mask[j] and j * S < ln for j in range(k))


def mask_of(n, lost):
    return [0 if j in lost else 1 for j in range(n)]


SWEEPS = [
    (4, 2, [1, 2, 3, 5, 16, 17, 31, 32, 33, 63, 64, 65, 100, 129],
     [(), (0,), (1,), (2,), (3,), (0, 1), (1, 3), (0, 4), (4, 5)]),
    (8, 3, [1, 17, 64, 65], [(), (0,), (7,), (3, 4), (0, 1, 2), (1, 5, 8), (8, 9, 10)]),
    (3, 2, [1, 5, 33, 64], [(), (0,), (1,), (2,), (0, 1), (1, 3), (3, 4)]),
]


@pytest.mark.parametrize("kind", ["stripes", "objects", "shards"])
@pytest.mark.parametrize("k,m,sizes,losses", SWEEPS, ids=["4+2", "8+3", "3+2"])
def test_every_length(k, m, sizes, losses, kind):
    """One entry for every lens 0..k S of every S.  In call c the codeword of
    the i-th S has lost losses[(i + c) % len(losses)], so every call mixes the
    patterns and every S meets every loss; on a shards plan shard j lies at
    residue (c + j) % 4, so every shard meets every residue."""
    enc = RS.New(k, m)
    n = k + m
    for c in range(max(len(losses), 4)):
        arena, lens, masks, md5s = Arena(kind), [], [], []
        for i, S in enumerate(sizes):
            w = word(k, m, S)
            mask = mask_of(n, losses[(i + c) % len(losses)])
            for ln in range(k * S + 1):
                arena.put(w, mask, residue=c + i)
                lens.append(ln)
                masks.append(mask)
                md5s.append(w.md5(ln) if ln else None)
        plan = arena.build(enc)
        dig, bad = slots(len(lens))
        s0 = B.etag_plan_stats()
        plan.etag_mixed(masks, lens, digests=dig, expected=expected_of(md5s), bad=bad)
        check_slots(dig, bad, md5s)
        assert arena.unchanged()
        s1 = B.etag_plan_stats()
        spec = [(arena.spec[e][-1], lens[e], masks[e]) for e in range(len(lens))]
        # nothing is decoded for all-present, for parity-only, or where the missing shard lies wholly beyond lens
        assert s1["decoded_entries"] - s0["decoded_entries"] == sum(model_decoded(k, S, ln, mk) for S, ln, mk in spec)
        assert s1["chains"] - s0["chains"] == sum(1 for ln in lens if ln)
        assert s1["kernel_launches"] - s0["kernel_launches"] == 1
        if kind != "shards":  # a healthy entry is ONE segment; a decoded one at most three
            healthy = sum(1 for S, ln, mk in spec if ln and not model_decoded(k, S, ln, mk))
            degraded = sum(1 for S, ln, mk in spec if model_decoded(k, S, ln, mk))
            assert healthy + degraded <= s1["segments"] - s0["segments"] <= healthy + 3 * degraded
            if degraded == 0:
                assert s1["segments"] - s0["segments"] == healthy


@pytest.mark.parametrize("kind", ["stripes", "objects"])
def test_all_present_slot_plans_walk_one_segment_per_entry(kind):
    k, m = 4, 2
    enc = RS.New(k, m)
    arena, lens, md5s = Arena(kind), [], []
    for i, S in enumerate([1, 17, 64, 100]):
        for ln in range(k * S + 1):
            arena.put(word(k, m, S), [1] * 6, residue=i)
            lens.append(ln)
            md5s.append(word(k, m, S).md5(ln) if ln else None)
    plan = arena.build(enc)
    for present in (None, [[1] * 6] * len(lens), [[1, 1, 1, 1, 0, 0]] * len(lens)):  # parity never matters
        dig, bad = slots(len(lens))
        s0 = B.etag_plan_stats()
        plan.etag_mixed(present, lens, digests=dig)
        check_slots(dig, bad, md5s)
        s1 = B.etag_plan_stats()
        assert s1["segments"] - s0["segments"] == s1["chains"] - s0["chains"] == sum(1 for ln in lens if ln)
        assert s1["decoded_entries"] == s0["decoded_entries"]
    assert arena.unchanged()


def _files_arena(k, m, chunk, lengths, lost_of):
    """Objects as their ec_split shard files in one device buffer.  lost_of(g,
    t) -> the shard files whose stripe t of object g is lost (GARBAGE there)."""
    img, objs, files, present = bytearray(b"\x3c" * 64), [], [], []
    for g, L in enumerate(lengths):
        obj = bytes(np.asarray(O.object_bytes(4100 + 17 * g + chunk, L), np.uint8)) if L else b""
        shard_files = [bytearray(f) for f in O.ec_split(k, m, obj, chunk)]
        sizes = O._stripe_sizes(k, chunk, L) if L else []
        for t, S in enumerate(sizes):
            lost = lost_of(g, t)
            for j in lost:
                shard_files[j][t * chunk:t * chunk + S] = bytes([GARBAGE] * S)
            present.append(mask_of(k + m, lost))
        offs = []
        for j, f in enumerate(shard_files):
            while len(img) % 4 != (g + j) % 4:
                img.append(GAP)
            offs.append(len(img))
            img += f + bytes([GAP] * 3)
        objs.append(obj)
        files.append((offs, L))
    dev = torch.from_numpy(np.frombuffer(bytes(img), np.uint8).copy()).cuda()
    base = dev.data_ptr()
    return dev, dev.clone(), objs, [([base + o if L else 0 for o in offs], L) for offs, L in files], present


@pytest.mark.parametrize("chunk", [1, 2, 5, 64, 70])
def test_files(chunk):
    k, m = 4, 2
    enc = RS.New(k, m)
    kc = k * chunk
    lengths = [1, kc - 1, kc, 0, kc + 1, 2 * kc + 3, 3 * kc + k]  # 2 kc + 3: the three-stripe reference case
    states = {"healthy": lambda g, t: (),
              "a file lost in every stripe": lambda g, t: ((g % k,) if g % 2 else (g % k, k + g % m)),
              "a file lost in one stripe only": lambda g, t: ((t + g) % k,) if t == g % 3 else ()}
    for name, lost_of in states.items():
        dev, copy, objs, files, present = _files_arena(k, m, chunk, lengths, lost_of)
        plan = B.StripePlan(enc, files=files, chunk_size=chunk)
        assert plan.object_start[-1] == len(present)
        assert plan.object_start[6] - plan.object_start[5] == 3
        md5s = [hashlib.md5(o).digest() if o else None for o in objs]  # the ETag: md5(obj)
        dig, bad = slots(len(lengths))
        s0 = B.etag_plan_stats()
        plan.etag_files(present if present else None, digests=dig, expected=expected_of(md5s), bad=bad)
        check_slots(dig, bad, md5s)
        assert torch.equal(dev, copy), name
        s1 = B.etag_plan_stats()
        assert s1["chains"] - s0["chains"] == sum(1 for L in lengths if L)
        lost_entries = sum(1 for row in present if not all(row[:k]))
        assert s1["decoded_entries"] - s0["decoded_entries"] <= lost_entries
        assert (s1["decoded_entries"] > s0["decoded_entries"]) == (name != "healthy")


def test_waves_of_mixed_lengths_and_a_deep_chain():
    """300 objects of 0..40 KiB in one call: the lanes of a wave differ in trip
    count over several waves, a third of them with a data shard lost.  Then
    chains of 1 MiB, healthy and degraded, for many ping-pong rounds."""
    k, m = 4, 2
    enc = RS.New(k, m)
    rng = np.random.default_rng(11)
    lens = [int(x) for x in rng.integers(0, 40 * 1024 + 1, 300)]
    lens[:8] = [0, 1, 63, 64, 65, 40 * 1024, 40 * 1024 - 1, 4096]
    for kind in ("stripes", "shards"):
        arena, masks, md5s = Arena(kind), [], []
        for e, ln in enumerate(lens):
            w = word(k, m, (ln + k - 1) // k, seed=9000 + e)
            masks.append(mask_of(6, ((e % k,) if e % 3 == 0 else ())))
            arena.put(w, masks[-1], residue=e)
            md5s.append(w.md5(ln) if ln else None)
        plan = arena.build(enc)
        dig, bad = slots(len(lens))
        plan.etag_mixed(masks, lens, digests=dig, expected=expected_of(md5s), bad=bad)
        check_slots(dig, bad, md5s)
        assert arena.unchanged()
    big = word(k, m, 256 * 1024, seed=9900)
    arena = Arena("stripes")
    lens = [1024 * 1024, 1024 * 1024 - 5, 7]
    masks = [mask_of(6, ()), mask_of(6, (1, 5)), mask_of(6, (0,))]
    for e in range(3):
        arena.put(big, masks[e], residue=e)
    plan = arena.build(enc)
    md5s = [big.md5(ln) for ln in lens]
    dig, bad = slots(3)
    plan.etag_mixed(masks, lens, digests=dig, expected=expected_of(md5s), bad=bad)
    check_slots(dig, bad, md5s)
    assert arena.unchanged()


@pytest.mark.parametrize("kind", ["stripes", "shards"])
def test_compare_sees_one_flipped_bit_at_every_position_below_lens(kind):
    """One entry per flipped bit, all with the true ETag as expected.  Healthy:
    a flip below lens sets that entry's bad, a flip at or beyond lens or in a
    parity shard sets nothing.  Shard 1 lost (survivors 0, 2, 3 and parity 4):
    a flip in shard 1 is a flip in garbage nobody reads, a flip in any survivor
    at position q changes the decoded byte S + q, a flip in parity 5 nothing."""
    k, m, S, ln = 4, 2, 20, 70
    enc = RS.New(k, m)
    w = word(k, m, S)
    for lost in ((), (1,)):
        mask = mask_of(6, lost)
        arena, wrong = Arena(kind), set()
        arena.put(w, mask)
        for j in range(k + m):
            for q in range(S):
                e = arena.put(w, mask, residue=j + q, flip=(j, q, (j + q) % 8))
                if j in lost or j == 5:
                    continue
                # shard 1 lost: byte q of EVERY survivor (0, 2, 3 and parity 4) enters the decoded byte S + q,
                # which lies below lens for every q, so a flip beyond lens in shard 3 shows there too
                if (S + q < ln) if lost else (j < k and j * S + q < ln):
                    wrong.add(e)
        n = len(arena.spec)
        plan = arena.build(enc)
        dig, bad = slots(n)
        plan.etag_mixed([mask] * n, [ln] * n, expected=expected_of([w.md5(ln)] * n), bad=bad)
        torch.cuda.synchronize()
        assert set(np.nonzero(bad.cpu().numpy() != BAD0)[0].tolist()) == wrong
        assert set(bad.cpu().numpy().tolist()) == {BAD0, BAD0 | 1}
        assert bytes(dig.cpu().numpy()) == bytes([DIG] * 16 * n)  # no digests asked for: none written
        assert arena.unchanged()
        # healthy: one per byte below lens; shard 1 lost: every byte of its four survivors
        assert len(wrong) == (4 * S if lost else ln)


def test_filter_leaves_unexamined_slots_untouched():
    k, m = 4, 2
    enc = RS.New(k, m)
    arena, lens, masks, md5s = Arena("stripes"), [], [], []
    filt = []
    for e in range(200):
        S = 1 + e % 37
        w = word(k, m, S)
        ln = (e * 7) % (k * S + 1)
        masks.append(mask_of(6, ((e % k,) if e % 2 else ())))
        arena.put(w, masks[-1], residue=e)
        lens.append(ln)
        filt.append([0, 1, 2, 3, 4][e % 5])
        md5s.append(w.md5(ln) if ln and filt[-1] & 2 else None)
    plan = arena.build(enc)
    dig, bad = slots(200)
    f = torch.tensor(filt, dtype=torch.int32, device="cuda")
    wrong = {e for e in range(200) if md5s[e] is not None and e % 3 == 0}
    exp = expected_of([None if e in wrong else d for e, d in enumerate(md5s)])
    plan.etag_mixed(masks, lens, digests=dig, expected=exp, bad=bad, filter=f, filter_bits=2)
    check_slots(dig, bad, md5s, wrong)
    assert torch.equal(f.cpu(), torch.tensor(filt, dtype=torch.int32)) and arena.unchanged()
    # a filter that passes nothing: nothing written
    dig, bad = slots(200)
    plan.etag_mixed(masks, lens, digests=dig, expected=exp, bad=bad, filter=f, filter_bits=8)
    check_slots(dig, bad, [None] * 200)

    # files: an object is hashed when ANY of its entries passes
    chunk = 5
    lengths = [3 * k * chunk + 2, 2 * k * chunk, 7, 4 * k * chunk]
    dev, copy, objs, files, present = _files_arena(k, m, chunk, lengths, lambda g, t: (1,) if t == 1 else ())
    fplan = B.StripePlan(enc, files=files, chunk_size=chunk)
    starts = fplan.object_start.tolist()
    fw = [0] * starts[-1]
    fw[starts[0] + 3] = 1  # object 0: its last entry only
    fw[starts[3]] = 1      # object 3: its first
    fw[starts[1]] = 2      # object 1: another bit
    md5s = [hashlib.md5(objs[0]).digest(), None, None, hashlib.md5(objs[3]).digest()]
    dig, bad = slots(4)
    fplan.etag_files(present, digests=dig, expected=expected_of([md5s[0], None, None, None]), bad=bad,
                     filter=torch.tensor(fw, dtype=torch.int32, device="cuda"))
    check_slots(dig, bad, md5s, wrong={3})
    assert torch.equal(dev, copy)


def test_13_plus_3_decodes_entry_by_entry():
    k, m = 13, 3
    enc = RS.New(k, m)
    sizes = [1, 17, 64, 65, 130]
    for kind in ("stripes", "shards"):
        for lost in ((), (4,)):
            arena, lens, masks, md5s = Arena(kind), [], [], []
            for i, S in enumerate(sizes):
                w = word(k, m, S)
                for ln in (1, S, 4 * S, 4 * S + 1, 5 * S, k * S - 1, k * S):
                    masks.append(mask_of(k + m, lost))
                    arena.put(w, masks[-1], residue=i)
                    lens.append(ln)
                    md5s.append(w.md5(ln))
            plan = arena.build(enc)
            dig, bad = slots(len(lens))
            s0, r0 = B.etag_plan_stats(), B.glue_range_stats()
            plan.etag_mixed(masks, lens, digests=dig, expected=expected_of(md5s), bad=bad)
            check_slots(dig, bad, md5s)
            assert arena.unchanged()
            s1, r1 = B.etag_plan_stats(), B.glue_range_stats()
            want = sum(1 for e, ln in enumerate(lens) if lost and lost[0] * arena.spec[e][-1] < ln)
            assert s1["decoded_entries"] - s0["decoded_entries"] == want
            assert s1["kernel_launches"] - s0["kernel_launches"] == 1
            assert r1["kernel_launches"] == r0["kernel_launches"]  # the decode goes per entry: one apply each
            assert r1["per_stripe_calls"] - r0["per_stripe_calls"] == want


def test_stats_deltas_are_exact():
    k, m = 4, 2
    enc = RS.New(k, m)
    sizes, lens = [10, 0, 33, 64, 7], [40, 0, 100, 129, 0]
    for kind in ("stripes", "shards"):
        arena = Arena(kind)
        lost1 = mask_of(6, (1,))
        for e, S in enumerate(sizes):
            arena.put(word(k, m, S), lost1 if e in (2, 3) else [1] * 6, residue=e)
        plan = arena.build(enc)
        md5s = [word(k, m, S).md5(ln) if ln else None for S, ln in zip(sizes, lens)]
        dig, bad = slots(5)
        s0 = B.etag_plan_stats()
        plan.etag_mixed(None, [40, 0, 0, 0, 0], digests=dig)
        s1 = B.etag_plan_stats()
        assert {key: s1[key] - s0[key] for key in s0} == {
            "kernel_launches": 1, "chains": 1, "segments": 1 if kind == "stripes" else 4, "decoded_entries": 0}
        masks = [[1] * 6, [1] * 6, lost1, lost1, lost1]
        plan.etag_mixed(masks, lens, digests=dig)
        s2 = B.etag_plan_stats()
        # entry 2 (S 33, 100 bytes): shard 0, the span [33, 66), the run behind it: 3 segments on both kinds but
        # stripes merges shards 2.. into one run, as rows walks shard 2 and the byte of shard 3 apart;
        # entry 3 (S 64, 129 bytes): shard 0, the span, and one byte of shard 2
        want = {"stripes": 1 + 3 + 3, "shards": 4 + (1 + 1 + 2) + (1 + 1 + 1)}[kind]
        assert {key: s2[key] - s1[key] for key in s0} == {
            "kernel_launches": 1, "chains": 3, "segments": want, "decoded_entries": 2}
        check_slots(dig, bad, md5s)
        assert arena.unchanged()


def test_length_errors_on_the_device():
    assert EH.length_errors()
