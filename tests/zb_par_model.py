"""What zip(back)'s whole-GPU decode (cniic_amd/csrc/k_zipback_par.hip, zb_par.hpp) must do with a stream, computed from the stream
alone: the serial loop's verdict, the depth of the text's copies below the capacity, the jump rounds, and whether the route takes the
stream or hands it back.  tests/test_zip_back_par.py holds the GPU to it, tests/test_zip_back_par_cpu.py holds it to zip_back_ref."""
import struct

import numpy as np

DONE, BAD_EXPLICIT, BAD_LOOKBACK = 1, 2, 3
MAX_ROUNDS = 32
SCAN_TILE = 2048            # kZbpTile: stream positions per block of the prefix sum
SCAN_BLOCK = 1024           # kZbpScanThreads: tiles per pass of the one block that sums the tiles


def jump_rounds(depth):
    """ceil(log2(depth + 1)): zbp_jump_rounds"""
    return int(depth).bit_length()


def walk(stream, need=None, cap=None):
    """the contract's loop -> dict(status, p, made, symbols, longest, depth, text): depth and text cover the bytes below cap"""
    n = len(stream)
    need = (1 << 64) - 1 if need is None else need
    sp = o = symbols = longest = 0
    room = 1 << 16
    text = np.zeros(room, np.uint8)
    depth = np.zeros(room, np.int64)
    src = np.frombuffer(bytes(stream), np.uint8)
    while True:
        if o >= need or sp + 2 > n:
            status = DONE
            break
        head = stream[sp] | (stream[sp + 1] << 8)
        ln = head & 0x7FFF
        if head & 0x8000:
            if sp + 4 > n:
                status = DONE
                break
            back = stream[sp + 2] | (stream[sp + 3] << 8)
            if back > o:
                status = BAD_LOOKBACK
                break
            k = min(ln, back)
        else:
            if sp + 2 + ln > n:
                status = BAD_EXPLICIT
                break
            k = ln
        keep = k if cap is None else max(0, min(k, cap - o))
        while o + keep > room:
            text = np.concatenate([text, np.zeros(room, np.uint8)])
            depth = np.concatenate([depth, np.zeros(room, np.int64)])
            room *= 2
        if head & 0x8000:
            text[o:o + keep] = text[o - back:o - back + keep]
            depth[o:o + keep] = depth[o - back:o - back + keep] + 1
            sp += 4
        else:
            text[o:o + keep] = src[sp + 2:sp + 2 + keep]
            sp += 2 + ln
        longest = max(longest, 4 if head & 0x8000 else 2 + ln)
        o += k
        symbols += 1
        if not k:
            status = DONE
            break
    below = o if cap is None else min(o, cap)
    return dict(status=status, p=sp, made=o, symbols=symbols, longest=longest, depth=int(depth[:below].max()) if below else 0, text=text[:below].tobytes())


def plan(stream, need=None, cap=None, floor=0, round_cap=MAX_ROUNDS):
    """-> walk()'s dict + routed, handed, rounds (the jump rounds the route runs on it)"""
    w = walk(stream, need, cap)
    n = len(stream)
    w["routed"] = 1 <= n < (1 << 32) and n >= floor
    w["handed"] = False
    w["rounds"] = 0
    if w["routed"] and w["status"] == DONE:
        own = jump_rounds(w["depth"])
        w["handed"] = own > min(round_cap, MAX_ROUNDS) or min(w["made"], (1 << 64) if cap is None else cap) >= (1 << 32)
        w["rounds"] = min(own, round_cap, MAX_ROUNDS)
    return w


def chain(n_lookbacks, length=8, back=8, head=b"abcdefgh"):
    """explicit(head) and N look-backs of (length, back): the last byte is N copies away from a literal when length == back == len(head)"""
    return struct.pack("<H", len(head)) + head + struct.pack("<HH", 0x8000 | length, back) * n_lookbacks


def long_text_stream(seed_bytes):
    """about 4 KB of stream that spell a little over 30 MB: 512 literal bytes, six look-backs that double the text, 960 of 32767 bytes"""
    assert len(seed_bytes) == 512
    out, o = struct.pack("<H", 512) + seed_bytes, 512
    while o < 32767:
        out += struct.pack("<HH", 0x8000 | o, o)
        o *= 2
    return out + struct.pack("<HH", 0x8000 | 32767, 32767) * 960
