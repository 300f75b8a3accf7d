"""Huffman streams built by hand for the GPU parse of a serialised decoder (cniic_amd/csrc/k_trieparse.hip): the dimensions, a pre-order
trie of any shape and an MSB-first payload that names every leaf, so that the image is known without any decoder.  A plain Python
parse of the same bytes gives what a case is named for: where every leaf record lies, how deep it is, at which offset the first tag of
every 1024-byte chunk stands, which node is a branch's right child, how deep the parser's stack gets.

tests/test_trie_shapes_cpu.py asserts, from this parse and from the oracle alone, that every case sits on the limit it names;
tests/test_trie_shapes.py decodes the same streams on the GPU.  This module imports no GPU code.

The limits are the library's (cited where they are restated; test_trie_shapes_cpu.py compares them with the sources):
    CHUNK      = 1024   kTpChunk      k_trieparse.hip   bytes per chunk of the maps
    MAX_LEN    = 56     kLeafMaxLen   huff_host.hpp     the deepest leaf the table of leaves holds
    MAX_P      = 120    kTpMaxP       k_trieparse.hip   the deepest stack the node records hold (7 bits next to the leaf flag)
    GROUP      = 64     the fan-in of k_tp_levels / k_tp_parents: nodes 64, 4096 and 262144 open a group of level 0, 1 and 2
    BATCH      = 8      kTpB          k_trieparse.hip   maps a thread of k_tp_chain_entries loads at a time
    CHAIN      = 1024   the threads of k_tp_chain_entries, and the chunks per block of k_tp_bases_*
    R          = 12 / 7 1 + huff_symbol_size(): a leaf record of `hufman` (tag, u64 length 3, r g b) and of `delta` (tag, three i16)
    FIRST_LOOK = max(nbytes / 48, 8192), 4 MiB at most: what codec_decode (codec.cpp) lets the host parse first
    MIN_SYMS   = 2^14   gpu_decode_min_symbols (codec.cpp): images below it never reach the GPU parse without a hook"""
import functools

import numpy as np

CHUNK = 1024
MAX_LEN = 56
MAX_P = 120
GROUP = 64
BATCH = 8
CHAIN = 1024
R_RGB, R_SIGNED = 12, 7
POS0 = 8                 # the trie follows the two u32 dimensions
MIN_SYMS = 1 << 14
PARSE, PARSE_HOST = "trie_parse", "trie_parse_host"

LEAF = None              # a shape is LEAF or a pair (left shape, right shape)


def first_look(nbytes):
    return min(max(nbytes // 48, 8192), 4 << 20)


# ------------------------------------------------------------------ shapes
def balanced(lo, hi=None):
    """the trie over leaves lo .. hi - 1 (or 0 .. lo - 1) split in halves, the larger half on the left"""
    n = lo if hi is None else hi - lo
    assert n >= 1
    if n == 1:
        return LEAF
    a = (n + 1) // 2
    return (balanced(a), balanced(n - a))


def right_comb(n):
    """n leaves at depths 1, 2, ..., n - 1, n - 1: every left child a leaf"""
    s = LEAF
    for _ in range(n - 1):
        s = (LEAF, s)
    return s


def left_comb(n):
    """n leaves, every right child a leaf: n - 1 branch tags, two leaves at depth n - 1, then the others from the bottom up"""
    s = LEAF
    for _ in range(n - 1):
        s = (s, LEAF)
    return s


def over(k, shape):
    """k leading branch tags whose right leaves come at the end: every record of `shape` lies k bytes later"""
    for _ in range(k):
        shape = (shape, LEAF)
    return shape


def walk(shape):
    """pre-order -> (tags, leaves): tags[i] = 1 for a branch and 0 for a leaf, leaves = [(depth, path as an integer of depth bits)]"""
    tags, leaves, todo = [], [], [(shape, 0, 0)]
    while todo:
        s, d, code = todo.pop()
        if s is LEAF:
            tags.append(0)
            leaves.append((d, code))
        else:
            tags.append(1)
            todo.append((s[1], d + 1, code << 1 | 1))
            todo.append((s[0], d + 1, code << 1))
    return tags, leaves


def graft(comb, subtree):
    """the shape with `subtree` in place of its deepest leaf (the last of them in pre-order)"""
    _, leaves = walk(comb)
    depth = max(d for d, _ in leaves)
    code = [c for d, c in leaves if d == depth][-1]
    path, s = [], comb
    for k in range(depth):
        bit = code >> (depth - 1 - k) & 1
        path.append((s, bit))
        s = s[bit]
    assert s is LEAF
    new = subtree
    for s, bit in reversed(path):
        new = (s[0], new) if bit else (new, s[1])
    return new


def beside(shape, n=700):
    """a root whose left child is balanced(n) and whose right child is `shape`: a decoder of more than 8192 bytes with every leaf of
    the shape one level deeper -- and BEHIND the host's first look at the stream (13 n - 1 > 8192), which would otherwise meet a branch
    at depth 56 itself and never ask the GPU"""
    return (balanced(n), shape)


def random_shape(leaves, seed, skew, cap=MAX_LEN):
    """random splits: one side gets 1 + (n - 2) u^skew of a node's n leaves (u uniform; either side), no leaf deeper than cap"""
    rng = np.random.default_rng(seed)

    def rec(n, d):
        if n == 1:
            return LEAF
        lim = 1 << min(cap - d - 1, 40)           # leaves one child can still hold
        assert n <= 2 * lim
        a = min(1 + int((n - 1) * rng.random() ** skew), n - 1)
        if rng.random() < 0.5:
            a = n - a
        a = min(max(a, n - lim, 1), n - 1, lim)
        return (rec(a, d + 1), rec(n - a, d + 1))
    return rec(leaves, 0)


# ------------------------------------------------------------------ streams
def _bits(s):
    s += "0" * (-len(s) % 8)
    return int(s, 2).to_bytes(len(s) // 8, "big") if s else b""


def rgb_record(key):
    return b"\x00\x03\x00\x00\x00\x00\x00\x00\x00" + int(key).to_bytes(3, "big")     # ser.rs:188-222: tag, u64 length, r g b


def signed_record(d):
    return b"\x00" + b"".join(int(v).to_bytes(2, "little", signed=True) for v in d)   # tag, three i16 (hilbertc.rs:561-571)


def delta_symbols(n):
    """n differences in pairs +v, -v (v >= 0 in every component, all v distinct), a zero difference last where n is odd"""
    out = []
    for j in range(n // 2):
        v = (1 + j % 255, j // 255 % 256, j // 65280)
        out += [v, tuple(-x for x in v)]
    if n % 2:
        out.append((0, 0, 0))
    return out


def fit(leaves, margin=0, at_least=(8, 8)):
    """the smallest of a few image sizes with room for every leaf (and `margin` more symbols)"""
    for w, h in ((8, 8), (20, 16), (67, 61), (128, 128), (300, 200), (512, 512)):
        if w * h >= leaves + margin and w * h >= at_least[0] * at_least[1]:
            return w, h
    raise AssertionError("no image for %d leaves" % leaves)


class Stream:
    """data: the stream; image: what it decodes to, from the payload alone (`hufman`) or None (`delta`: the oracle's decode);
    seq: the leaf of every symbol; the facts of parse()"""

    def __init__(self, codec, shape, dims=None, colours=None, ends_deepest=False, pad=b""):
        self.codec = codec
        rgb = codec == "hufman"
        self.R = R_RGB if rgb else R_SIGNED
        tags, leaves = walk(shape)
        n = len(leaves)
        self.leaves, self.deepest = n, max(d for d, _ in leaves)
        self.w, self.h = dims or fit(n, 2 if ends_deepest else 0)
        px = self.w * self.h
        deep = max(i for i in range(n) if leaves[i][0] == self.deepest)
        if rgb:
            syms = list(colours) if colours is not None else list(range(n))
            recs = [rgb_record(k) for k in syms]
        else:
            if colours is not None:
                syms = list(colours)
            elif ends_deepest:        # (the deepest leaf opens the payload: the zero difference, so that the colour stays inside 0 .. 255)
                rest = delta_symbols(n - 1)
                syms = rest[:deep] + [(0, 0, 0)] + rest[deep:]
            else:
                syms = delta_symbols(n)
            recs = [signed_record(d) for d in syms]
        assert len(syms) == n
        self.syms = syms
        it = iter(recs)
        trie = b"".join(b"\x01" if t else next(it) for t in tags)
        assert len(trie) == self.R * n + n - 1
        # the payload: the leaves in pre-order, again and again; with the deepest leaf in front and behind where a case wants that
        if ends_deepest:
            assert px >= n + 2
            seq = np.concatenate([[deep], np.arange(px - 2) % n, [deep]])
        else:
            assert px >= n
            seq = np.arange(px) % n
        self.seq = seq
        codes = [format(c, "0%db" % d) if d else "" for d, c in leaves]
        payload = _bits("".join([codes[i] for i in seq.tolist()]))
        self.trie_len = len(trie)
        self.payload_pos = POS0 + len(trie)
        self.data = self.w.to_bytes(4, "little") + self.h.to_bytes(4, "little") + trie + payload + pad
        self.image = None
        if rgb:
            keys = np.asarray(syms, np.uint32)[seq]
            self.image = np.stack([keys >> 16, keys >> 8 & 255, keys & 255], 1).astype(np.uint8).reshape(self.h, self.w, 3)

    def keys(self):
        """the library's 32-bit key of every symbol of the payload: r g b in 24 bits, or three differences + 255 in 9 bits each"""
        if self.codec == "hufman":
            per_leaf = np.asarray(self.syms, np.uint32)
        else:
            per_leaf = np.asarray([(a + 255) << 18 | (b + 255) << 9 | (c + 255) for a, b, c in self.syms], np.uint32)
        return per_leaf[self.seq]

    @property
    def on_gpu(self):
        """the route: the GPU's table answers iff no leaf lies deeper than the table holds"""
        return self.deepest <= MAX_LEN

    @property
    def natural(self):
        """the single decode reaches the GPU parse with no hook: the decoder outgrows the host's first look, the image is large enough"""
        return self.codec == "hufman" and self.w * self.h >= MIN_SYMS and self.payload_pos > first_look(len(self.data))


class Facts:
    pass


def parse(data, R, pos0=POS0):
    """a plain parse of the pre-order trie at data[pos0:] -> Facts: leaves [(offset of the record's tag, depth)], payload (offset
    behind the trie), entries (per chunk up to the trie's end, the offset in it of its first tag), right (per node, the node number
    of its right child, -1 for a leaf), max_p (the most subtrees open in front of a node: the parser's stack, the root counted)"""
    f = Facts()
    f.leaves, f.entries, f.right = [], [], []
    pos, pending, p, f.max_p = pos0, [(0, -1)], 1, 0      # pending: (depth, the branch whose right child this node is or -1)
    while pending:
        depth, parent = pending.pop()
        if pos >= len(data):
            raise ValueError("the trie does not end inside the stream")
        c = (pos - pos0) // CHUNK
        if c == len(f.entries):
            f.entries.append((pos - pos0) % CHUNK)
        assert c == len(f.entries) - 1                    # (a record is shorter than a chunk: no chunk without a tag)
        node = len(f.right)
        if parent >= 0:
            f.right[parent] = node
        f.max_p = max(f.max_p, p)
        tag = data[pos]
        if tag == 1:
            f.right.append(-1)
            pending += [(depth + 1, node), (depth + 1, -1)]
            pos += 1
            p += 1
        elif tag == 0:
            if pos + R > len(data):
                raise ValueError("cut inside a leaf")
            f.right.append(-1)
            f.leaves.append((pos, depth))
            pos += R
            p -= 1
        else:
            raise ValueError("tag %d" % tag)
    f.payload = pos
    f.nodes = len(f.right)
    f.deepest = max(d for _, d in f.leaves)
    return f


def tag_offsets(f, R, pos0=POS0):
    """the offset of every node's tag: a leaf's record, or the single byte of a branch"""
    out, pos, leaf_at = [], pos0, {o for o, _ in f.leaves}
    while pos < f.payload:
        out.append(pos)
        pos += R if pos in leaf_at else 1
    return out


def straddlers(f, R, pos0=POS0):
    """the leaf records (offsets of their tags) that lie across a chunk boundary"""
    return [o for o, _ in f.leaves if (o - pos0) // CHUNK != (o - pos0 + R - 1) // CHUNK]


# ------------------------------------------------------------------ the cases
END_LEAVES = (709, 394, 1103, 788, 473, 1182, 867, 552, 1261, 946, 631, 316)     # 13 n - 1 = r modulo 1024 for r = 0 .. 11
CHUNK_COUNTS = (1024, 1025, 8192, 8193)
RIGHT_N = (31, 32, 33, 2047, 2048, 2049, 131071, 131072, 131073)
DEPTHS = (55, 56, 57, 58, 64, 65, 119, 120, 121, 128, 300)
COMB_LEAVES = 45         # a comb of 45 leaves: its deepest at 44, and balanced(3000) below it reaches 44 + 12 = 56


def _comb(kind, deepest):
    return (right_comb if kind == "right" else left_comb)(deepest + 1)


@functools.lru_cache(maxsize=None)
def random_shapes():
    """[(seed, skew, shape, deepest leaf)] of random_shape(5000, seed, skew) for seeds 1 .. 6 at skew 3 and 8: those with the deepest leaf at 50 .. 56"""
    out = []
    for skew in (3, 8):
        for seed in range(1, 7):
            s = random_shape(5000, seed, skew)
            deepest = max(d for d, _ in walk(s)[1])
            if 50 <= deepest <= MAX_LEN:
                out.append((seed, skew, s, deepest))
    return out


@functools.lru_cache(maxsize=None)
def geometry_cases():
    """{name: Stream}, `hufman`: the chunk geometry"""
    c = {}
    for k in range(13):
        c["entry over(%d)" % k] = Stream("hufman", over(k, balanced(400)))
        c["entry over(%d), 700 leaves" % k] = Stream("hufman", over(k, balanced(700)), dims=(128, 128))     # (long enough for the natural gate)
    for n in END_LEAVES + (708, 710):
        c["end %d leaves" % n] = Stream("hufman", balanced(n), dims=(128, 128))
    for n in (1, 2, 78, 79):
        c["short %d leaves" % n] = Stream("hufman", balanced(n), colours=[0x0A0B0C] if n == 1 else None)
    return c


@functools.lru_cache(maxsize=None)
def chunk_count_cases():
    """{name: Stream}: balanced(8000) in front of 128 x 128 pixels, padded to a span of exactly 1024 / 1025 / 8192 / 8193 chunks and one byte more"""
    base = Stream("hufman", balanced(8000), dims=(128, 128))
    c = {}
    for chunks in CHUNK_COUNTS:
        for more in (0, 1):
            for fill in ((0, 1) if chunks == 8193 and not more else (0,)):
                s = Stream.__new__(Stream)
                s.__dict__.update(base.__dict__)
                s.data = base.data + bytes([fill]) * (POS0 + chunks * CHUNK + more - len(base.data))
                c["span %d chunks + %d, padded with %d" % (chunks, more, fill)] = s
    return c


@functools.lru_cache(maxsize=None)
def search_cases():
    """{name: Stream}, `hufman`: the right-child search"""
    c = {}
    for n in RIGHT_N:
        c["right child at node %d" % (2 * n)] = Stream("hufman", (balanced(n), balanced(100)), dims=fit(n + 100, at_least=(128, 128)))
        if 13 * (n + 100) < 8192:                     # (the same right child in a decoder long enough for the natural gate)
            c["right child at node %d, 700 leaves behind" % (2 * n)] = Stream("hufman", (balanced(n), balanced(700)), dims=(128, 128))
    c["left comb over 3000"] = Stream("hufman", graft(left_comb(COMB_LEAVES), balanced(3000)), dims=(128, 128))
    c["right comb over 3000"] = Stream("hufman", graft(right_comb(COMB_LEAVES), balanced(3000)), dims=(128, 128))
    for seed, skew, shape, _ in random_shapes():
        c["random seed %d skew %d" % (seed, skew)] = Stream("hufman", shape, dims=(128, 128))
    c["a colour twice"] = Stream("hufman", balanced(4), colours=[5, 6, 5, 7])
    return c


@functools.lru_cache(maxsize=None)
def depth_cases():
    """{name: Stream}, `hufman`: combs with the deepest leaf at DEPTHS, alone in front of a small image (the hook's runs) and beside
    balanced(700) in front of 128 x 128 (the natural gate's); the payload starts and ends with the deepest leaf"""
    c = {}
    for kind in ("right", "left"):
        for d in DEPTHS:
            c["%s comb %d" % (kind, d)] = Stream("hufman", _comb(kind, d), ends_deepest=True)
            c["%s comb %d beside 700" % (kind, d)] = Stream("hufman", beside(_comb(kind, d - 1)), dims=(128, 128), ends_deepest=True)
    return c


def knob_cases():
    """the streams with a 56-bit code that go through every decoder knob"""
    d, s = depth_cases(), search_cases()
    rnd = next("random seed %d skew %d" % (seed, skew) for seed, skew, _, deepest in random_shapes() if deepest == MAX_LEN)
    return {n: c for n, c in (("right comb 56", d["right comb 56"]), ("left comb 56", d["left comb 56"]), (rnd, s[rnd]))}


KNOBS = [{"CNIIC_HD_LUT3": a, "CNIIC_HD_KEEP": b} for a in "01" for b in "01"] + [{"CNIIC_HD_LUT2_BITS": "13"}, {"CNIIC_HD_LUT1": "0"}, {"CNIIC_HD_PHASES": "1"}]


@functools.lru_cache(maxsize=None)
def good_hufman():
    c = {}
    for part in (geometry_cases(), chunk_count_cases(), search_cases(), depth_cases()):
        assert not set(c) & set(part)
        c.update(part)
    return c


def _boundaries(s):
    return [POS0 + CHUNK * c for c in range(1, (s.payload_pos - POS0 + CHUNK - 1) // CHUNK)]   # the chunk starts inside the trie


def _put(data, at, byte):
    return data[:at] + bytes([byte]) + data[at + 1:]


def _malformed(s, more_leaf):
    """[(name, stream)] edits and cuts of the good stream s (over(k, balanced(n))): what the issue's list of malformed streams names"""
    data, f = s.data, parse(s.data, s.R)
    alltags = tag_offsets(f, s.R)
    spots = [("first byte", POS0), ("last leaf's tag", f.leaves[-1][0])]
    for b in _boundaries(s):
        spots.append(("last tag before %d" % b, max(t for t in alltags if t < b)))
        spots.append(("first tag from %d" % b, min(t for t in alltags if t >= b)))
    out = []
    for what, at in spots:
        for tag in (2, 255):
            out.append(("tag %d in the %s" % (tag, what), _put(data, at, tag)))
    o = straddlers(f, s.R)[0]
    for k in range(8):
        out.append(("length byte %d of the straddling record" % k, _put(data, o + 1 + k, 1 if k else 4)))
    last = f.leaves[-1][0]
    for at in range(last, last + s.R):
        out.append(("cut at byte %d of the last record" % (at - last), data[:at]))
    for b in _boundaries(s):
        for at in range(b - 12, b + 13):
            out.append(("cut at %d, boundary %d" % (at, b), data[:at]))
    out.append(("cut behind the trie", data[:f.payload]))
    out.append(("cut one byte into the payload", data[:f.payload + 1]))
    out.append(("a trie that never ends", data[:POS0] + b"\x01" * 2000))
    out.append(("one more leaf behind the trie", data[:f.payload] + more_leaf + data[f.payload:]))
    return out


@functools.lru_cache(maxsize=None)
def malformed_base():
    return Stream("hufman", over(3, balanced(400)))


@functools.lru_cache(maxsize=None)
def malformed_hufman():
    return _malformed(malformed_base(), rgb_record(0xABCDEF))


# ---- `delta`: 7-byte records
@functools.lru_cache(maxsize=None)
def good_delta():
    c = {}
    for k in range(8):
        c["delta entry over(%d)" % k] = Stream("delta", over(k, balanced(600)))
    for n in (32, 2048):
        c["delta right child at node %d" % (2 * n)] = Stream("delta", (balanced(n), balanced(100)))
    for kind in ("right", "left"):
        for d in (56, 57):
            c["delta %s comb %d" % (kind, d)] = Stream("delta", _comb(kind, d), ends_deepest=True)
    return c


@functools.lru_cache(maxsize=None)
def delta_base():
    return Stream("delta", over(3, balanced(600)))


@functools.lru_cache(maxsize=None)
def malformed_delta():
    """a straddling leaf whose component is 256 / -256 (each of the record's components that lies across the boundary or next to
    it), and the cuts of the last record"""
    s = delta_base()
    f = parse(s.data, s.R)
    out = []
    for o in straddlers(f, s.R)[:2]:
        for comp in range(3):
            for v in (256, -256):
                at = o + 1 + 2 * comp
                out.append(("component %d of the record at %d is %d" % (comp, o, v), s.data[:at] + int(v).to_bytes(2, "little", signed=True) + s.data[at + 2:]))
    last = f.leaves[-1][0]
    for at in range(last, last + s.R):
        out.append(("delta cut at byte %d of the last record" % (at - last), s.data[:at]))
    return out
