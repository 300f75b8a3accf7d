"""What the hand-built payloads of tests/payload_shapes.py are, without a GPU: from the oracle alone (its verdict, its pixels) and from the
plain bit walk (where every symbol boundary falls), so that tests/test_hd_payload.py can say which limit of k_hdecode.hip a failing case
sits on; the constants these tests restate against the source; and, for the streams that must never fall into step, decoders started at
the warm-up position of every subsequence.

If an assertion about a case's geometry fails, the case is to be mended, not the assertion: it is what puts the case on its limit."""
import os
import re

import numpy as np

import oracle_lib as O
import payload_shapes as P
import trie_shapes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _src(*path):
    return open(os.path.join(ROOT, *path)).read()


def test_the_constants_the_tests_restate_are_the_library_s():
    hd, cc = _src("cniic_amd", "csrc", "k_hdecode.hip"), _src("cniic_amd", "csrc", "codec.cpp")

    def const(name):
        m = re.search(r"constexpr \w+ %s = ([^;]+);" % name, hd)
        assert m, name
        return m.group(1).strip()
    assert const("kHdSub") == str(P.SUB) and const("kHdThreads") == str(P.BLOCK) and const("kHdKeep") == str(P.KEEP)
    assert int(const("kHdTail")) * 32 == P.TAIL and const("kHdLut") == str(P.LUT1)
    assert const("kHd3MaxBits") == str(P.LUT3_BITS) and const("kHd3MaxLeaves") == str(P.LUT3_LEAVES)
    assert "(n >= (1u << 20) ? %du : %du)" % (P.LUT2_CAP_BIG, P.LUT2_CAP) in hd and P.BIG_LEAVES == 1 << 20
    assert "max_len > (uint32_t)kHdLut ? std::min<uint32_t>(max_len, std::max(cap, (uint32_t)kHdLut + 1)) : 0u" in hd
    assert "if (bits2 > 20) {" in hd and const("kHdOwnMax") == "64"
    assert "nph = std::min(32u, std::max(16u, lt.max_len)), spb = kHpThreads / nph" in hd and [P.phases(m) for m in (7, 16, 17, 32, 56)] == [16, 16, 17, 32, 32]
    assert re.search(r"kHpGroups = %d;" % P.GROUPS, hd) and re.search(r"kHpThreads = %d," % P.HP_THREADS, hd) and "if (S.bit0 >= nph)" in hd
    assert const("kHdPhasesMaxSub") == "1ull << 16" and P.PHASES_MAX_SUB == 1 << 16 and "nsub <= kHdPhasesMaxSub || phases_force" in hd
    assert const("kHdBlindChecks") == str(P.BLIND) and const("kHdMaxPasses") == str(P.MAX_PASSES)
    assert const("kHdMaxRounds") == str(P.ROUNDS) and const("kHdRoundsShort") == str(P.ROUNDS_SHORT)
    assert "const bool wide = lt.max_len > %d;" % P.WIDE in hd
    assert "S.warm = payload_bytes * 8 >= nsyms * 12 ? 384 : 128;" in hd and (P.warm(1200, 100), P.warm(1199, 100)) == (384, 128)
    assert "S.bit0 = (a & 3) * 8;" in hd
    assert "nsyms * kHdSub <= payload_bytes * 8 * 48" in hd and P.keeps(512, 48) and not P.keeps(512, 49)
    assert "return bits2 == 0 || payload_bits * 2 < nsyms * 25;" in hd and P.first_table(24, 2, 16) and not P.first_table(25, 2, 16)
    assert "hopeless_pct ? std::max(1u, grid / 4) : 0u" in hd and [P.hopeless_min(n) for n in (1, 1792, 1793, 2048, 2049)] == [1, 1, 2, 2, 2]
    assert "return nsub <= (1ull << 16) ? 35u : nsub <= (1ull << 19) ? 60u : 97u;" in hd and [P.hopeless_pct(n) for n in (1 << 16, (1 << 16) + 1, (1 << 19) + 1)] == [35, 60, 97]
    assert "round == 3 && nl0 >= 64 && nl * 100 > nl0 * hopeless_pct" in hd
    assert "constexpr uint32_t kUdChunk = kUdThreads * kUdPer;" in hd and "static_assert(kUdChunk == %d" % P.CHUNK in hd
    api, readme = _src("include", "cniic_hip.h"), _src("README.md")
    for name in P.MARKS:
        assert 'ktimes["%s"]' % name in (cc if name == "hd_host_walk" else hd) and '"%s"' % name in api and "`%s`" % name in readme, name
        assert "CNIIC_TEST_" not in name
    for case in list(P.kept_cases().values()) + list(P.locked_cases().values()) + list(P.sixteen_cases().values()):
        for k in case.knobs:
            assert '"%s"' % k in hd, k


def test_the_builder_builds_what_it_says():
    m = P.mix()
    assert sorted((l, len(i)) for l, i in m.of_len.items()) == [(1, 1), (2, 1), (4, 2), (8, 31), (16, 256)] and m.n == 291
    assert [m.leaf(c) for c in ("0", "10", "1100", "1101", "11100000")] == [0, 1, 2, 3, 4] and m.leaf("1" * 16) == 290
    assert len(set(m.keys.tolist())) == m.n
    assert not m.diffs.sum(axis=0).any() and not m.diffs[[0, 1, 289, 290]].any()                     # +v / -v pairs; the zero differences
    assert m.diffs[m.leaf(P.ONE)].tolist() == [1, 1, 1] and m.diffs[m.leaf(P.BIG) + 1].tolist() == [-255] * 3
    for ml in (16, 17, 31, 32):
        s = P.seven(ml)
        assert s.max_len == ml and len(s.of_len[7]) == 127 and s.n == 127 + ml - 6 and "1111111" not in s.by_code
    x, xw = P.sixteen(), P.sixteen(40)
    assert x.max_len == 16 and len(x.of_len[16]) == 256 and x.n == 324 and (xw.max_len, xw.n) == (40, 362)
    assert all(("0000" + format(v >> 4, "04b") + "0000" + format(v & 15, "04b")) in x.by_code for v in range(256))
    assert 8 + len(x.trie("hufman")) < 8192 and 8 + len(xw.trie("hufman")) < 8192 and 8 + len(m.trie("hufman")) < 8192   # the host's first look holds the decoder
    for count in (32, 33, 63, 64, 65, 200, 511, 512):
        pt = P.pattern(count)
        assert len(pt) == count and sum(pt) == P.SUB and set(pt) <= {1, 2, 4, 8, 16}
    assert P.fill(131071, 7, 8).sum() == 131071 and P.fill(131071, 16, 15).sum() == 131071
    # a stream by hand: MIX, the symbols 0 10 1100 11100000 and the all-ones code
    p = P.Payload("hufman", m, [0, 1, 2, 4, 290], (5, 1), trailing=b"\x80", bit0=8)
    assert p.data[p.payload_pos:] == bytes([0b01011001, 0b11000001, 0b11111111, 0b11111110, 0x80]) and p.seq_bits == 31
    # (behind them one bit of padding, a 0, and the trailing byte: 10 and six times 0)
    assert p.bounds.tolist() == [8, 9, 11, 15, 23, 39, 40, 42, 43, 44, 45, 46, 47, 48] and p.chain.tolist() == [0, 1, 2, 4, 290, 0, 1] + [0] * 6 and p.nbits == 48 and p.nsub == 1 and p.end == 48
    assert p.count.tolist() == [13] and p.first.tolist() == [8, 48] and p.index.tolist() == [0]
    assert p.image.reshape(-1, 3).tolist() == [[k >> 16, k >> 8 & 255, k & 255] for k in m.keys[[0, 1, 2, 4, 290]].tolist()]
    assert P.pack(m.L, m.C, np.asarray([3, 0, 290])).tolist() == [1, 1, 0, 1, 0] + [1] * 16
    # the packer against a symbol-by-symbol one, codes of up to 56 bits
    c = P.comb(56)
    seq = np.random.default_rng(5).integers(0, c.n, 3000)
    assert "".join(map(str, P.pack(c.L, c.C, seq, chunk=1000).tolist())) == "".join(format(int(c.C[i]), "0%db" % c.L[i]) for i in seq)


def _plain_walk(p):
    """every symbol of the payload, bit by bit, from the bytes of the stream"""
    bits = "".join(format(b, "08b") for b in p.data[p.payload_pos:])
    at, out, starts = 0, [], []
    while at < len(bits):
        for l in range(1, p.fam.max_len + 1):
            i = p.fam.by_code.get(bits[at:at + l]) if at + l <= len(bits) else None
            if i is not None:
                break
        if i is None:
            break
        out.append(i)
        starts.append(p.bit0 + at)
        at += p.fam.L[i]
    return out, starts, p.bit0 + at


def _all_cases():
    out = {}
    for fn in (P.kept_cases, P.ends_cases, P.fromdiff_cases, P.locked_cases, P.sixteen_cases, P.first_table_cases):
        for n, c in fn().items():
            assert n not in out
            out[n] = c
    return out


def _oracle_agrees(name, p):
    rc, px = O.decode(p.codec, p.data)
    assert (rc == 0) == p.ok and rc in (0, O.DECODE), (name, rc)
    if rc == 0:
        assert px.shape == (p.h, p.w, 3)
        if p.codec == "hufman":
            assert np.array_equal(px, p.image), name
        else:
            assert np.array_equal(O.hilbert_linearize(px).astype(np.int64), p.lin), name


def test_streams_are_what_they_claim():
    """the oracle decodes every stream to the builder's image, or refuses where the case says so; the facts are those of a plain walk"""
    cases = _all_cases()
    assert len(cases) == 22 + 68 + 17 + 15 + 6 + 2
    walked = 0
    for name, case in cases.items():
        p = case.p
        _oracle_agrees(name, p)
        assert p.nbits == p.bit0 + 8 * (len(p.data) - p.payload_pos) and p.nsub == -(-p.nbits // P.SUB)
        assert p.count.sum() == len(p.chain) and len(p.count) == len(p.first) - 1 == len(p.over) == len(p.index) == p.nsub
        if p.nbits <= 1 << 17 or "16385" in name:
            out, starts, end = _plain_walk(p)
            assert out == p.chain.tolist() and starts == p.starts.tolist() and end == p.end, name
            t = np.asarray(starts) // P.SUB
            assert np.array_equal(np.bincount(t, minlength=p.nsub), p.count), name
            assert all(p.first[k] == min([s for s in starts + [end] if s >= k * P.SUB], default=p.nbits) for k in range(0, p.nsub, 7)), name
            walked += 1
    assert walked >= 100


def _in_step(p):
    """which subsequences t >= 1 the warm-up of pass 0 enters on a true boundary"""
    arrive, _, _ = p.warm_starts()
    return arrive == p.first[1:p.nsub]


def test_ordinary_streams_are_in_step_after_their_warm_up():
    """what hd_phases == 0 and hd_recheck == 0 rest on: every subsequence of these streams is entered where its predecessor ends, or is
    put right by its block's own settle loop in pass 0 (a few subsequences of one block, fewer than the verdict's 64)"""
    for fn in (P.kept_cases, P.ends_cases, P.fromdiff_cases, P.first_table_cases):
        for name, case in fn().items():
            p = case.p
            if p.nsub < 2:
                continue
            out = np.flatnonzero(~_in_step(p)) + 1
            if "stale" in name:
                assert out.tolist() == [P.STALE_T], name
            elif name.startswith("SEVEN"):
                assert len(out) <= 8 and p.nsub <= 9, name                   # (one block: settled before pass 0 ends)
            else:
                assert len(out) == 0, (name, out[:8])


def test_kept_symbol_cases():
    k = P.kept_cases()
    for codec in ("hufman", "delta"):
        p = k[codec + " counts natural"].p
        counts = p.count.tolist()
        assert counts[:20] == [32, 59, 32, 60, 32, 61, 32, 63, 32, 64, 32, 65, 32, 512, 32, 33, 34, 35, 512, 65] and not p.over.any()
        assert {P.KEEP - 1, P.KEEP, P.KEEP + 1, P.SUB} <= set(counts) and all(counts[i - 1] == 32 == counts[i + 1] for i in (7, 9, 11, 13))
        assert {c % 4 for c in counts if c <= P.KEEP} == {0, 1, 2, 3}                                  # the last, partial group of hd_run<STORE>
        assert p.end == p.nbits == p.nsub * P.SUB and p.nsyms == len(p.seq)
        p = k[codec + " borders natural"].p
        kept = p.count <= P.KEEP
        into_long = {int(p.index[t]) % 4 for t in range(1, p.nsub) if kept[t - 1] and not kept[t]}
        into_kept = {int(p.index[t]) % 4 for t in range(1, p.nsub) if not kept[t - 1] and kept[t]}
        assert into_long == into_kept == {0, 1, 2, 3}
        p = k[codec + " stale natural"].p
        t = P.STALE_T
        arrive, _, _ = p.warm_starts()
        assert arrive[t - 1] == t * P.SUB and p.first[t] == t * P.SUB + 8                               # half a code out of step
        _, wrong, _ = p.run([arrive[t - 1]], (t + 1) * P.SUB)
        assert (int(wrong[0]), int(p.count[t])) == (40, 32) and wrong[0] <= P.KEEP                     # both kept: eight stale entries stay behind
        assert _in_step(p)[t - 2] and _in_step(p)[t]                                                   # the neighbours are right: the block's loop cures t alone
        for name in ("counts", "borders", "stale"):
            assert k["%s %s 1" % (codec, name)].p is k["%s %s natural" % (codec, name)].p and k["%s %s 1" % (codec, name)].marks["hd_compact"] == 1
            assert k["%s %s 0" % (codec, name)].marks["hd_compact"] == 0
        a, b = k[codec + " gate kept"].p, k[codec + " gate not kept"].p
        assert a.payload_bytes == b.payload_bytes == 20 * 64 and b.nsyms == a.nsyms + 1 == 961
        assert P.keeps(8 * a.payload_bytes, a.nsyms) and a.nsyms * P.SUB == 8 * a.payload_bytes * 48 and not P.keeps(8 * b.payload_bytes, b.nsyms)
        assert max(a.count) <= P.KEEP and max(b.count) <= P.KEEP


def test_boundaries_and_ends():
    e = P.ends_cases()
    for n in P.NSUBS:
        p = e["nsub %d" % n].p
        assert p.nsub == n and (p.end == p.nbits == n * P.SUB or n == 513)                 # ends on a subsequence boundary, at 256 and 512 on a block's
    assert e["nsub 513"].p.nbits == 512 * P.SUB + 104
    seen = set()
    for pad in range(1, 8):
        for fam, more in (("MIX", pad), ("SEVEN", pad // 7)):
            name = "%s, %d bits of padding" % (fam, pad)
            p = e[name].p
            assert p.seq_bits % 8 == 8 - pad and len(p.chain) == len(p.seq) + more and p.nsyms == len(p.seq), name
            assert not e[name + ", one symbol too few"].p.ok and e[name + ", one symbol too few"].p.nsyms == len(p.chain) + 1
            assert ((name + ", all that the tail decodes to") in e) == (more > 0)
            if more:
                q = e[name + ", all that the tail decodes to"].p
                assert q.ok and q.nsyms == len(p.chain) and q.data[8:] == p.data[8:]
                seen.add(q.nsyms % 4)
            seen.add(p.nsyms % 4)
    assert seen == {0, 1, 2, 3}                                                             # nsyms = 4 k + 1 .. 3: the last group of four reaches past the image
    assert P.mix().by_code["0"] == 0 and P.seven(16).by_code["0000000"] == 0               # the all-zero code: 1 bit, 7 bits
    for fill_byte, per_byte in ((0x00, 8.0), (0xFF, 0.5)):
        for nb in P.TRAIL:
            name = "%d trailing bytes of %02x" % (nb, fill_byte)
            p = e[name].p
            assert p.nsyms == 160 and len(p.chain) == 160 + int(nb * per_byte) and p.nsub == 4 + -(-nb * 8 // P.SUB), name
            assert not e[name + ", one symbol too few"].p.ok
    p = e["16385 trailing bytes of 00"].p
    assert p.nsub > P.BLOCK + 4 and p.count[4:4 + P.BLOCK].tolist() == [P.SUB] * P.BLOCK       # a whole block of symbols past nsyms
    for deep in (32, 56):
        p = e["a code of %d bits over the end of a subsequence and of a block" % deep].p
        assert p.fam.max_len == deep and p.nsub > P.BLOCK + 1
        for at in P.DEEP_AT:
            i = int(np.searchsorted(p.starts, at))
            t = at // P.SUB
            assert p.starts[i] == at == (t + 1) * P.SUB - 1 and p.fam.L[p.seq[i]] == deep and p.over[t] == deep - 1 < P.TAIL
        assert {at // P.SUB % P.BLOCK for at in P.DEEP_AT} == {99, P.BLOCK - 1}
    assert (P.comb(32).max_len > P.WIDE, P.comb(56).max_len > P.WIDE) == (False, True)


def test_fromdiff_cases():
    f = P.fromdiff_cases()
    p = f["borders natural"].p
    m = p.fam
    t = np.searchsorted(p.index, [4096, 8192, 12288], side="right") - 1                  # the subsequence that holds the first symbol of chunks 1, 2, 3
    assert p.index[t[0]] < 4095 and p.count[t[0]] <= P.KEEP                              # inside one kept subsequence
    assert p.index[t[1]] == 8192 and p.count[t[1]] <= P.KEEP and t[1] // 64 == (t[1] - 1) // 64     # between two subsequences of one wave
    assert p.index[t[2]] < 12287 and p.count[t[2]] == 200 > P.KEEP                       # inside a subsequence k_hd_write decodes again
    d = m.diffs[p.seq]
    for b in (4096, 8192, 12288):
        assert d[b - 1].tolist() == [1, 1, 1] and d[b].tolist() == [-1, -1, -1] and d[b + 1].any()
    assert p.lin.min() >= 0 and p.lin.max() <= 255 and p.nsyms == 12800 and P.keeps(8 * p.payload_bytes, p.nsyms)
    for k in "10":
        p = f["touches 0 and 255, keep %s" % k].p
        assert p.ok and p.lin.min() == 0 and p.lin.max() == 255 and p.lin[4095].tolist() == [255] * 3 and p.lin[4096].tolist() == [0] * 3 and p.lin[8191].tolist() == [255] * 3
        for at, what in ((4095, "the last of a chunk"), (4096, "the first of a chunk"), (8191, "the last pixel")):
            for v in ("-1", "256"):
                q = f["%s at %s, keep %s" % (v, what, k)].p
                assert not q.ok and q.lin[at].tolist() == [int(v)] * 3 and (q.lin[:at] >= 0).all() and (q.lin[:at] <= 255).all()
                assert q.nsyms == 8192 and at % P.CHUNK in (0, P.CHUNK - 1)


def test_the_image_of_1025_chunks():
    p = P.big_delta_case().p
    assert -(-p.nsyms // P.CHUNK) == 1025 and p.ok and p.count.max() == 128
    _oracle_agrees("2049 x 2048", p)
    assert _in_step(p).all()


def _locked_stretch(p):
    """the stretch of the payload covered by the locked symbols (all but the last one)"""
    return int(p.starts[0]), int(p.starts[-1])


def test_locked_seven_streams_stay_out_of_step():
    cases = {n: c for n, c in dict(P.locked_cases(), **P.long_locked_cases()).items() if n.startswith("SEVEN")}
    assert len(cases) == 15 + 2
    for name, case in cases.items():
        if "entry offset" in name:
            continue
        p = case.p
        lo, hi = _locked_stretch(p)
        ones = np.concatenate([[0], np.cumsum(p.pbits[:hi], dtype=np.int64)])
        assert (ones[lo + 7:hi + 1] - ones[lo:hi - 6] < 7).all(), name          # every 7-bit window of the stretch holds a 0: 7-bit symbols at every offset
        w = P.warm(8 * p.payload_bytes, p.nsyms)
        assert w == 128
        t = np.arange(1, p.nsub)
        right = (t * P.SUB - w - p.bit0) % 7 == 0                                # a guess is right iff it lies a multiple of 7 behind bit0
        step = max(1, p.nsub // 2048)                                            # (the longest streams: every 32nd subsequence bit by bit)
        pick = np.arange(0, p.nsub - 1, step)
        arrive, _, met = p.run((t * P.SUB - w)[pick], ((t + 1) * P.SUB)[pick], watch=(lo, hi))
        assert np.array_equal(met, right[pick]), name                           # 6 of 7 never stand on a true boundary inside the stretch
        assert abs(right.mean() - 1 / 7) < 0.01
        if step == 1:
            # every full block of k_hd_pass: at least 64 threads out of step and staying so: the verdict
            for b in range(p.nsub // P.BLOCK):
                assert (~right[max(b * P.BLOCK - 1, 0):(b + 1) * P.BLOCK - 1]).sum() >= 64 * 3
        assert -(-p.nsub // P.BLOCK) // 4 <= p.nsub // P.BLOCK
        assert case.marks["hd_phases"] == 1 and case.marks["hd_recheck"] == 0
    for max_len in (16, 17):
        for bit0 in (0, 8, 16, 24):
            p = cases["SEVEN(%d) at bit %d" % (max_len, bit0)].p
            assert p.nsub == 1000 and p.bit0 == bit0 and p.nsub % (P.HP_THREADS // P.phases(max_len)) and p.fam.L[p.seq[-1]] == max_len
    assert [P.HP_THREADS // P.phases(m) for m in (16, 17)] == [64, 60]
    assert [(b >= 16, b >= 17) for b in (0, 8, 16, 24)] == [(False, False), (False, False), (True, False), (True, True)]    # the launch for subsequence 0 alone
    assert sorted(c.p.nsub for n, c in cases.items() if n in P.long_locked_cases()) == [P.PHASES_MAX_SUB, P.PHASES_MAX_SUB + 1]     # the two sides of the gate
    for nsub in P.CHAIN_NSUBS + (P.PHASES_MAX_SUB, P.PHASES_MAX_SUB + 1):
        assert cases["SEVEN(16), %d subsequences" % nsub].p.nsub == nsub
    assert [-(-n // P.GROUPS) for n in P.CHAIN_NSUBS] == [1, 1, 2, 2, 3] and [n % -(-n // P.GROUPS) for n in (513, 1025)] == [1, 2]
    assert cases["SEVEN(16), %d subsequences" % (P.PHASES_MAX_SUB + 1)].p.nsyms > 4_600_000
    for max_len in (31, 32):
        case = cases["SEVEN(%d), entry offset %d" % (max_len, max_len - 1)]
        p = case.p
        i = int(np.searchsorted(p.starts, 3 * P.SUB - 1))
        assert p.starts[i] == 3 * P.SUB - 1 and p.fam.L[p.seq[i]] == max_len and p.over[2] == max_len - 1 and case.knobs == {"CNIIC_HD_PHASES": "1"}
    assert P.phases(32) - 1 == 31                                                # the largest entry a map holds


def test_no_guess_is_ever_right_on_a_sixteen_stream_at_bit_8():
    c = P.sixteen_cases()
    for name, case in c.items():
        p = case.p
        blocks = 60 if "60" in name else 40
        assert p.nsub == blocks * P.BLOCK + (1 if p.bit0 or "wide" in name else 0) and p.nsyms == blocks * P.BLOCK * 32
        assert set(p.data[p.payload_pos:-5]) <= set(range(16))                   # a string of bytes 0x0?
        w = P.warm(8 * p.payload_bytes, p.nsyms)
        assert w == 384
        t = np.arange(1, p.nsub)
        lo, hi = _locked_stretch(p)
        pick = np.unique(np.concatenate([np.arange(0, p.nsub - 1, 61), np.arange(P.BLOCK - 1, p.nsub - 1, P.BLOCK)]))    # every block's first subsequence among them
        arrive, _, met = p.run((t * P.SUB - w)[pick], ((t + 1) * P.SUB)[pick], watch=(lo, hi))
        if p.bit0 == 8:
            assert not met.any() and (arrive[arrive < hi] % 16 == 0).all() and (p.bounds[:-1] % 16 == 8).all(), name
        else:
            assert met.all() and np.array_equal(arrive, p.first[2:p.nsub + 1][pick]), name
        assert (p.fam.max_len > P.WIDE) == ("wide" in name)
        if "wide" in name:
            assert p.fam.L[p.seq[-1]] == 40 and (p.fam.L[p.seq[:-1]] == 16).all()
    # a block a check: block 0 in pass 0, blocks 1 and 2 in the blind checks, one more per looked check and a last one that finds nothing
    assert 41 - 1 - P.BLIND + 1 >= 30 and 41 - 1 <= P.MAX_PASSES and 61 - 1 > P.MAX_PASSES and P.ROUNDS >= P.BLOCK
    assert c["40 blocks at bit 8, no phase maps"].marks["hd_recheck"] == (">=", 30) and c["60 blocks at bit 8, no phase maps"].marks["hd_host_walk"] == 1
    assert c["wide, 60 blocks at bit 8"].marks["hd_host_walk"] == 1 and c["wide, 40 blocks at bit 8"].marks["hd_host_walk"] == 0 and not c["wide, 60 blocks at bit 8"].knobs


def test_sixteen_streams_on_the_two_sides_of_the_phase_map_gate():
    c = {n: v for n, v in P.long_locked_cases().items() if n.startswith("SIXTEEN")}
    a, b = c["SIXTEEN at bit 8, 65536 subsequences"], c["SIXTEEN at bit 8, 65537 subsequences"]
    assert (a.p.nsub, b.p.nsub) == (P.PHASES_MAX_SUB, P.PHASES_MAX_SUB + 1) and b.p.nsyms == a.p.nsyms + 1 and a.p.bit0 == b.p.bit0 == 8
    for case in (a, b):
        p = case.p
        _oracle_agrees("SIXTEEN", p)
        assert (p.bounds % 16 == 8).all() and (p.fam.L[p.seq] == 16).all() and P.warm(8 * p.payload_bytes, p.nsyms) % 16 == 0      # every guess 8 bits off
        t = np.arange(1, p.nsub, 257)
        _, _, met = p.run(t * P.SUB - 384, (t + 1) * P.SUB, watch=(0, p.nbits))
        assert not met.any()
    # the threads of a block are wrong but agree: one list entry a round, never the verdict's 64; a block is cured per check
    assert a.marks == {"hd_phases": 1, "hd_recheck": 0, "hd_host_walk": 0} and b.marks == {"hd_phases": 1, "hd_recheck": P.MAX_PASSES - P.BLIND, "hd_host_walk": 0}
    assert P.PHASES_MAX_SUB // P.BLOCK > P.MAX_PASSES


def test_verdict_cases():
    c = P.verdict_cases()
    assert [n.split()[0] for n in c] == ["0", "30", "256"]
    for K, case in zip(P.VERDICT_LOCKED, c.values()):
        p = case.p
        _oracle_agrees("verdict %d" % K, p)
        assert p.nsub == 1024 and P.hopeless_min(p.nsub) == 1 and p.nsub <= P.PHASES_MAX_SUB
        out = ~_in_step(p)
        per_block = [int(out[max(b * P.BLOCK - 1, 0):(b + 1) * P.BLOCK - 1].sum()) for b in range(4)]
        assert per_block[1:] == [0, 0, 0] and not out[K:].any()                       # the escape symbols fall into step at once
        if K:
            lo, hi = int(p.starts[0]), int(p.starts[K * P.SUB // 7])
            ones = np.concatenate([[0], np.cumsum(p.pbits[:hi], dtype=np.int64)])
            assert (ones[lo + 7:hi + 1] - ones[lo:hi - 6] < 7).all() and hi > (K - 1) * P.SUB
        if K == 256:
            assert per_block[0] >= 64 * 3 and case.marks["hd_phases"] == 1           # a list of 64 and more that keeps its length: the verdict
        else:
            # fewer than 64: no verdict; a chain of K cures at most: pass 0's rounds and the first blind check's
            assert per_block[0] == (K and per_block[0]) < 64 and K <= 2 * P.ROUNDS_SHORT and case.marks == {"hd_phases": 0, "hd_recheck": 0}
            assert (per_block[0] > 20) == (K > 0)


def test_table_cases():
    c = P.table_cases()
    assert len(c) == 10
    for name, (s, knobs) in c.items():
        rc, px = O.decode("hufman", s.data)
        assert rc == 0 and np.array_equal(px, s.image) and np.array_equal(np.unique(s.seq), np.arange(s.leaves)), name      # every leaf named
        assert 8 + s.trie_len < 8192
    bits2 = {d: P.lut2_bits(d, d + 1) for d in (12, 13, 18, 19, 24, 25)}
    assert bits2 == {12: 0, 13: 13, 18: 18, 19: 18, 24: 18, 25: 18}
    assert [c["deepest code %d" % d][0].deepest for d in (12, 13, 18, 19, 24, 25)] == [12, 13, 18, 19, 24, 25]
    assert 24 - P.LUT2_CAP == P.LUT3_BITS and 25 - P.LUT2_CAP == P.LUT3_BITS + 1                       # the prefix of 18 ones: a third table | the bisection
    for n in (P.LUT3_LEAVES, P.LUT3_LEAVES + 1):
        depths = [d for d, _ in S.walk(S.graft(S.right_comb(P.LUT2_CAP + 1), S.balanced(n)))[1]]
        assert sum(d > P.LUT2_CAP for d in depths) == n and c["%d leaves under one prefix" % n][0].leaves == P.LUT2_CAP + n and max(depths) - P.LUT2_CAP > P.LUT3_BITS
    one = [d for d, _ in S.walk(S.graft(S.right_comb(P.LUT2_CAP + 1), P.full(4)))[1]]
    assert {d for d in one if d > P.LUT2_CAP} == {22} and one.count(22) == 16
    s, knobs = c["a second table of 21 bits"]
    assert knobs == {"CNIIC_HD_LUT2_BITS": "21"} and s.deepest == 23 and P.lut2_bits(23, s.leaves, cap=21) == 21 > 20
    own = {d: 1 << (21 - d) for d in range(1, 22)}                                                      # prefixes a leaf of d bits owns
    assert own[15] == 64 and own[14] == 128 and own[1] == 1 << 20                                       # kHdOwnMax: all its own | the rest to k_hd_lut_owner_big
    a, b = (v.p for v in P.first_table_cases().values())
    assert a.payload_bytes == b.payload_bytes == 1600 and (a.nsyms, b.nsyms) == (1024, 1025)
    assert not P.first_table(8 * a.payload_bytes, a.nsyms, 16) and P.first_table(8 * b.payload_bytes, b.nsyms, 16) and P.lut2_bits(16, 291) == 16


def test_the_small_streams_for_the_knobs():
    s = P.small_cases()
    assert len(s) == 12 and all(not c.knobs and c.p.ok and c.p.nsub <= 320 for c in s.values())
