"""Huffman streams built by hand for the parallel payload decoder (cniic_amd/csrc/k_hdecode.hip): a trie of a chosen shape, the key of
every leaf and an explicit symbol SEQUENCE -- the leaf of every pixel -- packed MSB-first, so that where every symbol boundary falls in
the payload is chosen and not met by chance.  Beside tests/trie_shapes.py, whose walk, records and shapes are used here, and whose Stream
always names "the leaves in pre-order, again and again".

A plain bit walk of the finished payload (Payload.walk: the listed symbols by their lengths, then whatever the padding and the trailing
bytes decode to, symbol by symbol) gives the facts a case is named for, per subsequence of SUB bits: how many symbols start in it, its
first boundary, the overshoot into the next one, the index of its first symbol; and the payload's bit length.  They are stated in the
decoder's frame: bits are counted from the 4-byte boundary below the payload's first byte WHERE THE DECODER READS IT (hd_stream:
bit0 = 8 * (address & 3)); a payload that comes as host bytes is copied to an aligned buffer and has bit0 = 0 (outside the forced GPU
parse), device bytes are placed at the residue that gives the case's bit0 (tests/test_hd_payload.py).

tests/test_hd_payload_cpu.py asserts from this walk and from the oracle alone that every case sits on the limit it names;
tests/test_hd_payload.py decodes the same streams on the GPU.  This module imports no GPU code.

The limits, all of cniic_amd/csrc/k_hdecode.hip (test_hd_payload_cpu.py compares them with the source):
    SUB            = 512    kHdSub           bits per subsequence, one thread each
    BLOCK          = 256    kHdThreads       subsequences per block of k_hd_pass / k_hd_write / k_hd_compact
    KEEP           = 64     kHdKeep          symbols kept per subsequence for k_hd_compact; a subsequence with more is decoded again
    TAIL           = 128    kHdTail * 32     bits staged past a block's last subsequence
    LUT1           = 12     kHdLut           bits of the first table
    LUT2 cap       = 18, 24 from 2^20 leaves (huff_decode_tables_dev: cap2); lut2_bits() = hd_lut2_bits
    LUT3           = 6 bits past the second table (kHd3MaxBits), 96 leaves under a prefix (kHd3MaxLeaves)
    phases         = min(32, max(16, max_len))   (phases(): nph), 1024 / phases subsequences per block of k_hd_phase_maps
    GROUPS         = 512    kHpGroups        groups of k_hd_phase_chain, ceil(nsub / 512) subsequences each
    PHASES_MAX_SUB = 2^16   kHdPhasesMaxSub  up to here the phase maps follow unsettled blind checks
    BLIND          = 2      kHdBlindChecks
    MAX_PASSES     = 48     kHdMaxPasses     checks in all before a stream is given up (wide codes: status 2, the host's walk)
    ROUNDS         = 320 / 24  kHdMaxRounds / kHdRoundsShort   rounds of a block's settle loop
    CHUNK          = 4096   kUdChunk         symbols per chunk of FromDiff's sums
    warm-up        = 384 if payload_bits >= 12 * nsyms else 128   (hd_stream)
    keep gate      = nsyms * 512 <= payload_bits * 48
    first table    = bits2 == 0 or payload_bits * 2 < nsyms * 25   (hd_use_first_table)
    verdict        = max(1, grid / 4) blocks whose out-of-step list (64 entries at least) keeps 35 / 60 / 97 % of its length over three
                     rounds (hd_hopeless_pct by nsub: up to 2^16, up to 2^19, beyond)"""
import functools

import numpy as np

import trie_shapes as T
from trie_shapes import LEAF

SUB, BLOCK, KEEP, TAIL, LUT1 = 512, 256, 64, 128, 12
LUT2_CAP, LUT2_CAP_BIG, BIG_LEAVES = 18, 24, 1 << 20
LUT3_BITS, LUT3_LEAVES = 6, 96
GROUPS, PHASES_MAX_SUB, BLIND, MAX_PASSES = 512, 1 << 16, 2, 48
ROUNDS, ROUNDS_SHORT, CHUNK, WIDE = 320, 24, 4096, 32
HP_THREADS = 1024
MARKS = ("hd_phases", "hd_recheck", "hd_compact", "hd_host_walk")


def phases(max_len):
    return min(32, max(16, max_len))


def warm(payload_bits, nsyms):
    return 384 if payload_bits >= 12 * nsyms else 128


def keeps(payload_bits, nsyms):
    return nsyms * SUB <= payload_bits * 48


def lut2_bits(max_len, leaves, cap=None):
    cap = cap or (LUT2_CAP_BIG if leaves >= BIG_LEAVES else LUT2_CAP)
    return min(max_len, max(cap, LUT1 + 1)) if max_len > LUT1 else 0


def first_table(payload_bits, nsyms, bits2):
    return bits2 == 0 or payload_bits * 2 < nsyms * 25


def hopeless_pct(nsub):
    return 35 if nsub <= 1 << 16 else 60 if nsub <= 1 << 19 else 97


def hopeless_min(nsub):
    return max(1, -(-nsub // BLOCK) // 4)


# ------------------------------------------------------------------ shapes
def full(d):
    return LEAF if d == 0 else (full(d - 1), full(d - 1))


def under(d, last, other=LEAF):
    """the full tree of depth d with `other` for every leaf and `last` for the all-ones one"""
    def rec(k, ones):
        if k == d:
            return last if ones else other
        return (rec(k + 1, False), rec(k + 1, ones))
    return rec(0, True)


class Family:
    """a trie and the symbol of every leaf (pre-order): `hufman` keys, all different, and `delta` differences that come in +v / -v
    pairs inside every code length (pair j of a length: its leaves 2 j and 2 j + 1; a leaf without a partner is the zero difference)"""

    def __init__(self, name, shape, special=()):
        self.name, self.shape = name, shape
        tags, leaves = T.walk(shape)
        self.tags, self.leaves = tags, leaves
        self.n = len(leaves)
        self.L = np.asarray([d for d, _ in leaves], np.int64)
        self.C = np.asarray([c for _, c in leaves], np.uint64)
        self.max_len = int(self.L.max())
        self.by_code = {format(c, "0%db" % d): i for i, (d, c) in enumerate(leaves)}
        self.of_len = {int(l): np.flatnonzero(self.L == l) for l in np.unique(self.L)}
        self.keys = ((np.arange(self.n, dtype=np.uint64) + 1) * 0x01F35B & 0xFFFFFF).astype(np.uint32)
        diffs = np.zeros((self.n, 3), np.int64)
        j = 0
        for l, idx in sorted(self.of_len.items()):
            for p in range(len(idx) // 2):
                v = (1 + j % 5, j // 5 % 5, j // 25 % 5)
                diffs[idx[2 * p]], diffs[idx[2 * p + 1]] = v, [-x for x in v]
                j += 1
        for code, v in special:                       # (code of the + leaf: its partner is the next leaf)
            i = self.by_code[code]
            assert self.L[i] == self.L[i + 1]
            diffs[i], diffs[i + 1] = v, [-x for x in v]
        self.diffs = diffs

    def leaf(self, code):
        return self.by_code[code]

    @functools.lru_cache(maxsize=None)
    def trie(self, codec):
        if codec == "hufman":
            recs = iter([T.rgb_record(k) for k in self.keys.tolist()])
        else:
            recs = iter([T.signed_record(d) for d in self.diffs.tolist()])
        return b"".join(b"\x01" if t else next(recs) for t in self.tags)

    def by_length(self, lengths, codec, pairs=4, fixed=None):
        """a leaf for every code length of `lengths`: `hufman` goes round the leaves of that length, `delta` takes +v, -v, +v' ... of
        its first `pairs` pairs, so that no colour ever leaves 0 .. 5 * pairs * (the lengths in use) -- or, pairs = 0, the zero
        difference of that length.  fixed {position: code}: those symbols as given (of the length the position has)"""
        lengths = np.asarray(lengths, np.int64)
        seq = np.full(len(lengths), -1, np.int64)
        for at, code in (fixed or {}).items():
            assert lengths[at] == len(code), (at, int(lengths[at]), code)
            seq[at] = self.by_code[code]
        for l in np.unique(lengths):
            at = np.flatnonzero((lengths == l) & (seq < 0))
            idx = self.of_len[int(l)]
            k = np.arange(len(at))
            if codec == "hufman":
                seq[at] = idx[k % len(idx)]
            elif pairs == 0 or len(idx) < 2:
                zero = idx[~self.diffs[idx].any(axis=1)]
                assert len(zero), l
                seq[at] = zero[k % len(zero)]
            else:
                seq[at] = idx[2 * (k // 2 % min(pairs, len(idx) // 2)) + k % 2]
        return seq


# MIX's last 16-bit pairs (the leaf named and the next one): +-(1, 1, 1), +-(255, 255, 255) and two zero differences (the all-ones code among them)
ONE, BIG, ZERO16 = "1111111111111000", "1111111111111010", "1111111111111110"


@functools.lru_cache(maxsize=None)
def mix():
    """codes of 1, 2, 4, 8 and 16 bits: 0, 10, 110x, 1110xxxx, 1111yyyy (yyyy < 15), 11111111 + 8 bits: 291 leaves"""
    return Family("MIX", (LEAF, (LEAF, (full(1), (full(4), under(4, full(8)))))), special=((ONE, (1, 1, 1)), (BIG, (255, 255, 255)), (ZERO16, (0, 0, 0))))


@functools.lru_cache(maxsize=None)
def seven(max_len):
    """127 leaves of 7 bits and a right comb under 1111111 whose two deepest leaves lie at max_len"""
    assert max_len >= 8
    return Family("SEVEN(%d)" % max_len, under(7, T.right_comb(max_len - 6)))


@functools.lru_cache(maxsize=None)
def sixteen(deep=None):
    """256 leaves 0000aaaa0000bbbb at depth 16, shallow leaves beside every 0 of the two runs (1, 01, 001, 0001 and 0000aaaa1 ...); with
    `deep`, a right comb in place of the leaf 01 whose two deepest leaves lie at `deep`"""
    x = under(4, T.over(4, full(4)), T.over(4, full(4)))
    n3 = (x, LEAF)
    n2 = (n3, LEAF)
    n1 = (n2, T.right_comb(deep - 1) if deep else LEAF)
    return Family("SIXTEEN(%s)" % deep, (n1, LEAF))


def locked_seven(fam, n, seed=1):
    """n 7-bit symbols whose middle bit is 0: every 7-bit window of their payload, at every offset, holds a 0, so that a decoder in a
    wrong phase reads 7-bit symbols only and keeps its phase"""
    codes = np.asarray([c for c in range(127) if not c >> 3 & 1])
    lut = np.asarray([fam.leaf(format(c, "07b")) for c in codes.tolist()])
    return lut[np.random.default_rng(seed).integers(0, len(lut), n)]


def locked_sixteen(fam, n, seed=1):
    """n symbols 0000aaaa0000bbbb: a string of bytes 0x0?, which reads as such symbols at byte offset 1 as well"""
    ab = np.random.default_rng(seed).integers(0, 256, n)
    lut = np.asarray([fam.leaf("0000" + format(v >> 4, "04b") + "0000" + format(v & 15, "04b")) for v in range(256)])
    return lut[ab]


@functools.lru_cache(maxsize=None)
def pattern(count, nbits=SUB):
    """`count` code lengths of 1, 2, 4, 8, 16 that add up to nbits, the longest first (as a tuple)"""
    c = {16: nbits // 16, 8: 0, 4: 0, 2: 0, 1: 0}
    rest, have = nbits % 16, nbits // 16
    for l in (8, 4, 2, 1):
        if rest >= l:
            c[l] += 1
            rest -= l
            have += 1
    assert have <= count <= nbits, (count, nbits)
    while have < count:
        l = max(k for k in c if c[k] and k > 1)
        c[l] -= 1
        c[l // 2] += 2
        have += 1
    return tuple(l for l in (16, 8, 4, 2, 1) for _ in range(c[l]))


def lengths(*parts):
    """the code lengths of a payload: every part a count of symbols for one whole subsequence, (count, nbits) for a stretch of nbits, or
    a list of lengths as they are"""
    out = []
    for p in parts:
        if isinstance(p, (int, np.integer)):
            out.append(pattern(int(p)))
        elif isinstance(p, tuple) and len(p) == 2 and p[1] > 16:
            out.append(pattern(*p))
        else:
            out.append(tuple(p))
    return np.concatenate([np.asarray(o, np.int64) for o in out])


# ------------------------------------------------------------------ the stream
def pack(L, C, seq, chunk=1 << 18):
    """the codes of seq, MSB-first -> (uint8 array of the bits, unpadded).  No loop over symbols: a stretch of `chunk` symbols at a time"""
    out = []
    for a in range(0, len(seq), chunk):
        s = seq[a:a + chunk]
        l, c = L[s], C[s]
        if l.min() == l.max():
            k = int(l[0])
            out.append(((c[:, None] >> np.arange(k - 1, -1, -1, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(np.uint8).ravel())
            continue
        first = np.cumsum(l) - l
        idx = np.repeat(np.arange(len(s)), l)
        j = np.arange(int(l.sum())) - first[idx]
        out.append(((c[idx] >> (l[idx] - 1 - j).astype(np.uint64)) & np.uint64(1)).astype(np.uint8))
    return np.concatenate(out) if out else np.zeros(0, np.uint8)


class Payload:
    """data: the stream; nsyms = w * h; chain: the leaf of every symbol the walk meets (seq, then what padding and trailing bytes decode
    to); ok: the reference decodes it (enough symbols; `delta`: no colour outside 0 .. 255); image (`hufman`) or lin (`delta`: the
    colours along the traversal, prefix sums of the differences) -- and the facts, in the frame of bit0:
    nbits, nsub, bounds (every symbol boundary of the chain, the end of its last symbol included), count[t], first[t], over[t] (the
    first boundary of subsequence t + 1 less its first bit), index[t] (the number of the first symbol that starts in t)"""

    def __init__(self, codec, fam, seq, dims, trailing=b"", bit0=0):
        self.codec, self.fam, self.bit0 = codec, fam, bit0
        self.w, self.h = dims
        self.nsyms = self.w * self.h
        seq = np.asarray(seq, np.int64)
        self.seq = seq
        bits = pack(fam.L, fam.C, seq)
        self.seq_bits = len(bits)
        payload = np.packbits(bits).tobytes() + bytes(trailing)
        trie = fam.trie(codec)
        self.payload_pos = T.POS0 + len(trie)
        self.data = self.w.to_bytes(4, "little") + self.h.to_bytes(4, "little") + trie + payload
        self.payload_bytes = len(payload)
        self.nbits = bit0 + 8 * len(payload)
        self.nsub = -(-self.nbits // SUB)
        self.pbits = np.concatenate([np.zeros(bit0, np.uint8), np.unpackbits(np.frombuffer(payload, np.uint8)), np.zeros(64, np.uint8)])   # the frame's bits (zeros in front and behind)
        self.walk()
        n = self.nsyms
        self.ok = len(self.chain) >= n
        self.image = self.lin = None
        if codec == "hufman":
            if self.ok:
                k = fam.keys[self.chain[:n]]
                self.image = np.stack([k >> 16, k >> 8 & 255, k & 255], 1).astype(np.uint8).reshape(self.h, self.w, 3)
        elif self.ok:
            self.lin = np.cumsum(fam.diffs[self.chain[:n]], axis=0)          # (int64: exact)
            self.ok = bool(self.lin.min() >= 0 and self.lin.max() <= 255)

    def walk(self):
        fam = self.fam
        l = fam.L[self.seq]
        starts = self.bit0 + np.concatenate([[0], np.cumsum(l)])
        at, tail, tail_at = int(starts[-1]), [], []
        pb = self.pbits
        while at < self.nbits:                      # padding and trailing bytes, bit by bit
            code, i = "", None
            while at + len(code) < self.nbits and len(code) < fam.max_len:
                code += "1" if pb[at + len(code)] else "0"
                i = fam.by_code.get(code)
                if i is not None:
                    break
            if i is None:
                break
            tail.append(i)
            at += len(code)
            tail_at.append(at)
        self.chain = np.concatenate([self.seq, np.asarray(tail, np.int64)])
        self.bounds = np.concatenate([starts, np.asarray(tail_at, np.int64)])      # (ascending: a code is at least one bit)
        self.starts = self.bounds[:-1]
        self.end = int(self.bounds[-1])
        t = np.arange(self.nsub + 1)
        at_t = np.searchsorted(self.starts, np.minimum(t * SUB, self.nbits))
        self.index = at_t[:-1]
        self.count = np.diff(at_t)
        b = np.searchsorted(self.bounds, t * SUB)
        self.first = np.where(b < len(self.bounds), self.bounds[np.minimum(b, len(self.bounds) - 1)], self.nbits)
        self.over = self.first[1:] - t[1:] * SUB

    # ---- decoders started anywhere
    @functools.cached_property
    def _len16(self):
        fam = self.fam
        W = min(fam.max_len, 16)
        tab = np.zeros(1 << W, np.int64)
        for d, c in fam.leaves:
            if d <= W:
                tab[c << (W - d):(c + 1) << (W - d)] = d
        return W, tab

    def lens_at(self, pos):
        """the length of the code that starts at every bit position of pos (0 where none ends inside the payload's 64 zeros)"""
        W, tab = self._len16
        pos = np.asarray(pos, np.int64)
        win = np.zeros(len(pos), np.int64)
        for k in range(W):
            win = win << 1 | self.pbits[np.minimum(pos + k, len(self.pbits) - 1)]
        out = tab[win]
        for i in np.flatnonzero(out == 0):           # deeper than the table: bit by bit
            code = ""
            while len(code) < self.fam.max_len and pos[i] + len(code) < len(self.pbits):
                code += "1" if self.pbits[pos[i] + len(code)] else "0"
                if code in self.fam.by_code:
                    out[i] = len(code)
                    break
        return out

    def run(self, at, until, watch=None):
        """decoders started at the positions `at`, each to its first boundary at or past `until` (or the payload's end) -> (where they
        arrive, the symbols each met, whether it stood on a true boundary inside watch = [lo, hi) on its way)"""
        at = np.array(at, np.int64)
        until = np.minimum(np.broadcast_to(np.asarray(until, np.int64), at.shape), self.nbits)
        is_b = np.zeros(self.nbits + 65, bool)
        is_b[self.bounds] = True
        met, cnt = np.zeros(len(at), bool), np.zeros(len(at), np.int64)
        live = at < until
        while live.any():
            i = np.flatnonzero(live)
            if watch is not None:
                met[i] |= is_b[at[i]] & (at[i] >= watch[0]) & (at[i] < watch[1])
            l = self.lens_at(at[i])
            stop = (l == 0) | (at[i] + l > self.nbits)
            at[i[stop]] = self.nbits
            at[i[~stop]] += l[~stop]
            cnt[i[~stop]] += 1
            live = at < until
        return at, cnt, met

    def warm_starts(self, watch=None):
        """pass 0 of k_hd_pass: where the warm-up of every subsequence t >= 1 arrives (subsequence 0 starts at bit0)"""
        t = np.arange(1, self.nsub)
        w = warm(8 * self.payload_bytes, self.nsyms)
        return self.run(t * SUB - w, t * SUB, watch)


# ------------------------------------------------------------------ the cases
class Case:
    """p: the Payload; knobs: the environment of the decode; marks: what the stage marks must say for device bytes at p.bit0 (a number,
    or (">=", n)); host_marks: the same for host bytes, which the decoder reads at bit0 = 0 (None: as marks where p.bit0 is 0, else
    nothing but the zeros every case demands)"""

    def __init__(self, p, knobs=None, marks=None, host_marks=None):
        self.p, self.knobs, self.marks = p, dict(knobs or {}), dict(marks or {})
        self.host_marks = dict(marks or {}) if host_marks is None and p.bit0 == 0 else dict(host_marks or {})


def rect(n):
    h = max(d for d in range(1, int(n ** 0.5) + 1) if n % d == 0)
    return n // h, h


def close(counts, least=8):
    """counts and one more subsequence of 32 .. 200 symbols, so that the total is w x h with h >= least"""
    for c in range(32, 200):
        if rect(sum(counts) + c)[1] >= least:
            return list(counts) + [c]
    raise AssertionError(counts)


def fill(nbits, a, b):
    """nbits as code lengths a and b (coprime), as few of b as possible, spread evenly"""
    nb = next(k for k in range(a) if (nbits - k * b) % a == 0 and nbits >= k * b)
    na = (nbits - nb * b) // a
    out = np.full(na + nb, a, np.int64)
    if nb:
        out[np.linspace(0, na + nb - 1, nb).astype(int)] = b
    return out


KEEP_KNOBS = ({}, {"CNIIC_HD_KEEP": "1"}, {"CNIIC_HD_KEEP": "0"})
SETTLED = {"hd_phases": 0, "hd_recheck": 0}      # an ordinary stream: in step after pass 0 and the blind checks
ALL_ONES = "1" * 16
STALE_T = 3


def _mix_payload(codec, counts, **kw):
    m = mix()
    L = lengths(*counts)
    return Payload(codec, m, m.by_length(L, codec), rect(len(L)), **kw)


def stale_lengths():
    """subsequence STALE_T lies in a run of the all-ones code that starts 8 bits off the 16-bit grid: its warm-up stays half a code out
    of step, falls into step on the eight zeros of 1111111100000000 INSIDE the subsequence and counts 40 symbols where there are 32"""
    head = [pattern(40)] * (STALE_T - 1)
    run = [(8,), (16,) * 48, (16,), (8,), (16,) * 14]
    L = lengths(*head, *run, *[pattern(40)] * 2, pattern(64))
    at = (STALE_T - 1) * 40 + 1
    fixed = {at + k: ALL_ONES for k in range(48)}
    fixed[at + 48] = "1111111100000000"
    return L, fixed


@functools.lru_cache(maxsize=None)
def kept_cases():
    c = {}
    m = mix()
    for codec in ("hufman", "delta"):
        streams = {
            "counts": _mix_payload(codec, close([32, 59, 32, 60, 32, 61, 32, 63, 32, 64, 32, 65, 32, 512, 32, 33, 34, 35, 512, 65])),
            "borders": _mix_payload(codec, close([33, 66] * 4 + [33, 67, 33, 67, 34, 65])),
        }
        L, fixed = stale_lengths()
        streams["stale"] = Payload(codec, m, m.by_length(L, codec, fixed=fixed), rect(len(L)))
        for name, p in streams.items():
            for knobs in KEEP_KNOBS:
                on = knobs.get("CNIIC_HD_KEEP", "01"[keeps(8 * p.payload_bytes, p.nsyms)]) == "1"
                c["%s %s %s" % (codec, name, knobs.get("CNIIC_HD_KEEP", "natural"))] = Case(p, knobs, dict(SETTLED, hd_compact=int(on)))
        # the natural gate: 20 subsequences of 48 symbols, and one symbol more in the same bits
        c["%s gate kept" % codec] = Case(_mix_payload(codec, [48] * 20), {}, dict(SETTLED, hd_compact=1))
        c["%s gate not kept" % codec] = Case(_mix_payload(codec, [48] * 19 + [49]), {}, dict(SETTLED, hd_compact=0))
    return c


NSUBS = (1, 255, 256, 257, 512, 513)
TRAIL = (1, 64, 65, 16385)
DEEP_AT = (100 * SUB - 1, BLOCK * SUB - 1)       # a deep code on the last bit of a subsequence inside a block, and of a block's last


@functools.lru_cache(maxsize=None)
def comb(deepest):
    """codes 0, 10, 110, ... up to `deepest` bits: any 0 ends a symbol, so every decoder is in step after one"""
    return Family("COMB(%d)" % deepest, T.right_comb(deepest + 1))


def _with_nsyms(p, n):
    """the same payload in front of another image size"""
    q = Payload.__new__(Payload)
    q.__dict__.update(p.__dict__)
    q.w, q.h = rect(n)
    q.nsyms = n
    q.data = q.w.to_bytes(4, "little") + q.h.to_bytes(4, "little") + p.data[8:]
    q.ok = len(q.chain) >= n
    q.image = None
    if q.ok:
        k = q.fam.keys[q.chain[:n]]
        q.image = np.stack([k >> 16, k >> 8 & 255, k & 255], 1).astype(np.uint8).reshape(q.h, q.w, 3)
    return q


def _ends(c, name, p):
    """p decodes len(seq) symbols; then every symbol the padding and the trailing bytes decode to as well; then one too many"""
    assert p.codec == "hufman"
    c[name] = Case(p, {}, dict(SETTLED))
    more = len(p.chain)
    if more > len(p.seq):
        c[name + ", all that the tail decodes to"] = Case(_with_nsyms(p, more), {}, {})
    c[name + ", one symbol too few"] = Case(_with_nsyms(p, more + 1), {}, {})


def straddle(fam, a, b, deep):
    """a code of `deep` bits on the last bit of subsequence 99 and of subsequence 255 (the last of block 0), lengths a and b around it"""
    parts, at = [], 0
    for pos in DEEP_AT:
        parts += [fill(pos - at, a, b), [deep]]
        at = pos + deep
    parts.append(fill(257 * SUB + 64 - at - (257 * SUB + 64 - at) % a, a, b))
    return np.concatenate([np.asarray(x, np.int64) for x in parts])


@functools.lru_cache(maxsize=None)
def ends_cases():
    c = {}
    m = mix()
    for n in NSUBS:
        counts = [40] * min(n, 512) + ([(7, 100)] if n == 513 else [])
        c["nsub %d" % n] = Case(_mix_payload("hufman", counts), {}, dict(SETTLED, hd_compact=1))
    c["nsub 256 delta"] = Case(_mix_payload("delta", [40] * 256), {}, dict(SETTLED, hd_compact=1))
    for pad in range(1, 8):
        L = lengths(40, 41, 40, [1] * (8 - pad))
        _ends(c, "MIX, %d bits of padding" % pad, Payload("hufman", m, m.by_length(L, "hufman"), rect(len(L))))
        s = seven(16)
        n = 584 + pad                                   # 7 n = -n modulo 8: n = pad modulo 8 leaves pad bits
        _ends(c, "SEVEN, %d bits of padding" % pad, Payload("hufman", s, np.arange(n) % 127, rect(n)))
    for fill_byte in (0x00, 0xFF):
        for nb in TRAIL:
            L = lengths(40, 40, 40, 40)
            _ends(c, "%d trailing bytes of %02x" % (nb, fill_byte), Payload("hufman", m, m.by_length(L, "hufman"), rect(len(L)), trailing=bytes([fill_byte]) * nb))
    for fam, a, b, deep in ((comb(32), 16, 15, 32), (comb(56), 16, 15, 56)):
        L = straddle(fam, a, b, deep)
        c["a code of %d bits over the end of a subsequence and of a block" % deep] = Case(Payload("hufman", fam, fam.by_length(L, "hufman"), rect(len(L))), {}, dict(SETTLED))
    return c


# ---- FromDiff on the way
def _border_lengths():
    """chunk borders (symbols 4096, 8192, 12288) inside a kept subsequence, between two subsequences, and inside a long one"""
    long_sub = (2,) * 90 + (4,) * 5 + (16,) * 4 + (2,) * 78 + (4,) * 23
    assert len(long_sub) == 200 and sum(long_sub) == SUB
    return lengths(*[40] * 103, *[40] * 101, 32, *[40] * 100, long_sub, 48, *[40] * 9)


@functools.lru_cache(maxsize=None)
def fromdiff_cases():
    c = {}
    m = mix()
    plus, minus = ONE, ONE[:-1] + "1"
    L = _border_lengths()
    fixed = {}
    for b in (4096, 8192, 12288):
        fixed[b - 1], fixed[b] = plus, minus
    p = Payload("delta", m, m.by_length(L, "delta", fixed=fixed), (128, 100))
    for knobs in KEEP_KNOBS:
        on = knobs.get("CNIIC_HD_KEEP", "01"[keeps(8 * p.payload_bytes, p.nsyms)]) == "1"
        c["borders %s" % knobs.get("CNIIC_HD_KEEP", "natural")] = Case(p, knobs, dict(SETTLED, hd_compact=int(on)))
    # colours at the edge of their range: nothing but zero differences around the symbols named
    L = lengths(*[40] * 204, 32)
    up, down, big, small = ONE, ONE[:-1] + "1", BIG, BIG[:-1] + "1"

    def edge(fixed):
        return Payload("delta", m, m.by_length(L, "delta", pairs=0, fixed=fixed), (128, 64))
    for knobs in ({"CNIIC_HD_KEEP": "1"}, {"CNIIC_HD_KEEP": "0"}):
        k = knobs["CNIIC_HD_KEEP"]
        c["touches 0 and 255, keep %s" % k] = Case(edge({4095: big, 4096: small, 4097: big, 8190: small, 8191: big}), knobs, dict(SETTLED, hd_compact=int(k)))
        for at, what in ((4095, "the last of a chunk"), (4096, "the first of a chunk"), (8191, "the last pixel")):
            c["-1 at %s, keep %s" % (what, k)] = Case(edge({at: down}), knobs, {})
            c["256 at %s, keep %s" % (what, k)] = Case(edge({10: big, at: up}), knobs, {})
    return c


@functools.lru_cache(maxsize=None)
def big_delta_case():
    """2049 x 2048: 1025 chunks, two per thread of k_ud_scan; 128 symbols a subsequence"""
    m = mix()
    L = np.tile(np.asarray(pattern(128), np.int64), 2049 * 2048 // 128)
    return Case(Payload("delta", m, m.by_length(L, "delta"), (2049, 2048)), {}, dict(SETTLED, hd_compact=0))


# ---- streams that never fall into step
PHASED = {"hd_phases": 1, "hd_recheck": 0, "hd_compact": 0}
CHAIN_NSUBS = (511, 512, 513, 1024, 1025)


def _locked_seven(max_len, nsub, bit0, last=True, seed=1):
    """a locked payload of exactly nsub subsequences at bit0; the deepest leaf once, at the very end"""
    s = seven(max_len)
    room = nsub * SUB - bit0 - (max_len if last else 0)
    n = room // 7
    while (7 * n + (max_len if last else 0) + 7) // 8 * 8 + bit0 > nsub * SUB:      # (whole bytes)
        n -= 1
    seq = locked_seven(s, n, seed)
    if last:
        seq = np.concatenate([seq, [int(s.of_len[max_len][-1])]])
    return Payload("hufman", s, seq, rect(len(seq)), bit0=bit0)


@functools.lru_cache(maxsize=None)
def locked_cases():
    c = {}
    for max_len in (16, 17):
        for bit0 in (0, 8, 16, 24):
            c["SEVEN(%d) at bit %d" % (max_len, bit0)] = Case(_locked_seven(max_len, 1000, bit0), {}, PHASED, host_marks=PHASED)
    for max_len in (31, 32):
        # a deepest code on the last bit of subsequence 2: entered max_len - 1 bits into subsequence 3
        s = seven(max_len)
        L = np.concatenate([fill(3 * SUB - 1, 7, 8), [max_len], fill(5 * SUB + 3, 7, 8)])
        c["SEVEN(%d), entry offset %d" % (max_len, max_len - 1)] = Case(Payload("hufman", s, s.by_length(L, "hufman"), rect(len(L))), {"CNIIC_HD_PHASES": "1"},
                                                                    {"hd_phases": 1, "hd_compact": 0})
    for nsub in CHAIN_NSUBS:
        c["SEVEN(16), %d subsequences" % nsub] = Case(_locked_seven(16, nsub, 0), {}, PHASED)
    return c


VERDICT_LOCKED = (0, 30, 256)     # subsequences of locked payload in front of 1024 (four blocks: the verdict wants max(1, 4 / 4) = 1 of them)


@functools.lru_cache(maxsize=None)
def verdict_cases():
    """SEVEN(16), 1024 subsequences: K of locked payload, then escape symbols (1111111 and a comb of 1 .. 9 bits: every decoder is in step
    within a symbol or two).  K = 0: nothing to settle.  K = 30: a list of fewer than 64 entries is no verdict, and a chain of 30 cures is
    done within pass 0's 24 rounds and the first blind check's.  K = 256: block 0 says hopeless, which is one block of four: the maps"""
    s = seven(16)
    esc = np.concatenate([s.of_len[l] for l in range(8, 17)])
    c = {}
    for K in VERDICT_LOCKED:
        n = K * SUB // 7
        room = 1024 * SUB - 7 * n
        e = esc[np.random.default_rng(3).integers(0, len(esc), room // 8)]
        e = e[:np.searchsorted(np.cumsum(s.L[e]), room - 16)]
        seq = np.concatenate([locked_seven(s, n), e])
        c["%d locked subsequences of 1024" % K] = Case(Payload("hufman", s, seq, rect(len(seq))), {}, PHASED if K == 256 else SETTLED)
    return c


@functools.lru_cache(maxsize=None)
def long_locked_cases():
    """65536 and 65537 subsequences, the two sides of the gate that sends a short stream to the phase maps after its blind checks.
    Locked SEVEN: every block says hopeless, so the maps follow pass 0 on both sides; past the gate (4.7 M symbols) that verdict alone
    leads there.  SIXTEEN at bit 8, one symbol apart: no block says so (the threads are wrong but agree among themselves: a list of one
    entry a round), and the blind checks end unsettled -- up to the gate the maps at once, past it 46 looked checks that cure a block
    each, then the maps"""
    c = {"SEVEN(16), %d subsequences" % nsub: Case(_locked_seven(16, nsub, 0), {}, PHASED) for nsub in (65536, 65537)}
    x = sixteen()
    none = {"hd_phases": 0, "hd_recheck": 0}
    for n, nsub, recheck in ((2097151, 65536, 0), (2097152, 65537, MAX_PASSES - BLIND)):
        p = Payload("hufman", x, locked_sixteen(x, n), rect(n), bit0=8)
        c["SIXTEEN at bit 8, %d subsequences" % nsub] = Case(p, {}, {"hd_phases": 1, "hd_recheck": recheck, "hd_host_walk": 0}, host_marks=none)
    return c


def _locked_sixteen(blocks, bit0, deep=None):
    x = sixteen(deep)
    n = blocks * BLOCK * SUB // 16
    seq = locked_sixteen(x, n)
    if deep:
        seq[-1] = int(x.of_len[deep][-1])
    return Payload("hufman", x, seq, rect(n), bit0=bit0)


@functools.lru_cache(maxsize=None)
def sixteen_cases():
    c = {}
    many = {"hd_phases": 0, "hd_recheck": (">=", 30), "hd_host_walk": 0}
    none = {"hd_phases": 0, "hd_recheck": 0, "hd_host_walk": 0}
    walk = {"hd_phases": 0, "hd_host_walk": 1}
    off = {"CNIIC_HD_PHASES": "0"}
    c["40 blocks at bit 8, no phase maps"] = Case(_locked_sixteen(40, 8), off, many, host_marks=none)
    c["40 blocks at bit 0, no phase maps"] = Case(_locked_sixteen(40, 0), off, none)
    c["60 blocks at bit 8, no phase maps"] = Case(_locked_sixteen(60, 8), off, walk, host_marks=none)
    c["wide, 40 blocks at bit 8"] = Case(_locked_sixteen(40, 8, deep=40), {}, many, host_marks=none)
    c["wide, 60 blocks at bit 8"] = Case(_locked_sixteen(60, 8, deep=40), {}, walk, host_marks=none)
    c["40 blocks at bit 8"] = Case(_locked_sixteen(40, 8), {}, {"hd_phases": 1, "hd_recheck": 0, "hd_host_walk": 0}, host_marks=none)
    return c


# ---- the tables: trie_shapes' shapes and Stream as they are, every leaf named by the payload
@functools.lru_cache(maxsize=None)
def table_cases():
    """{name: (Stream, knobs)}"""
    c = {}
    for deepest in (12, 13, 18, 19, 24, 25):
        c["deepest code %d" % deepest] = (T.Stream("hufman", T.right_comb(deepest + 1)), {})
    for n in (LUT3_LEAVES, LUT3_LEAVES + 1):
        c["%d leaves under one prefix" % n] = (T.Stream("hufman", T.graft(T.right_comb(LUT2_CAP + 1), T.balanced(n))), {})
    c["a prefix of one code length"] = (T.Stream("hufman", T.graft(T.right_comb(LUT2_CAP + 1), full(4))), {})
    c["a second table of 21 bits"] = (T.Stream("hufman", T.right_comb(24)), {"CNIIC_HD_LUT2_BITS": "21"})
    return c


@functools.lru_cache(maxsize=None)
def first_table_cases():
    """MIX (a second table of 16 bits), 12800 bits: 1024 symbols do not ask the first table, 1025 do"""
    return {"1024 symbols": Case(_mix_payload("hufman", [41] * 24 + [40]), {}, dict(SETTLED)),
            "1025 symbols": Case(_mix_payload("hufman", [41] * 25), {}, dict(SETTLED))}


def small_cases():
    """the small streams that go through trie_shapes.KNOBS once more"""
    k, e, f = kept_cases(), ends_cases(), fromdiff_cases()
    names = [n for n in k if n.endswith("natural")] + ["nsub 257", "MIX, 3 bits of padding", "SEVEN, 7 bits of padding, all that the tail decodes to", "65 trailing bytes of ff",
                                                       "a code of 56 bits over the end of a subsequence and of a block", "borders natural"]
    all_ = dict(k, **e, **f)
    return {n: all_[n] for n in names}
