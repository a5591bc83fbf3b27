"""Edge shapes of the device parser (csrc/hip/parse.hip), byte by byte.

test_gpu_parse.py reaches the parser's position-dependent branches only through random
files.  Here every input is built on purpose so that a terminator, a line start, a token
or a duplicate sits on a chosen boundary of the kernels -- 16 KB tiles cut from lo & ~63,
64-byte thread chunks, the 2 KB halo staged in front of a tile and the 64 bytes behind it,
the backward search for the previous line end, the unterminated tail line, the duplicate
filter / LDS column / scratch, the 256-line compaction chunk and its 4 x 64 gather -- and
every builder asserts that its bytes sit where its name says.

The expected result is a pure-Python statement of the input semantics (utils.jvm
split_lines / java_split_ws on the bytes as latin-1, first-occurrence dedup, repeats to
extras, the numeric rule "0" | [1-9][0-9]* <= 2^31 - 2 with id = value + 1, and "lines
starting in [b, e)" for byte ranges); it never calls the parsers.  Every comparison is
exact equality on the whole output: offsets, items, extras in order, vocabulary size and
the numeric / not-numeric decision (dictionary results through token bytes and hashes).

Every case runs on the host parser too (csrc/host/parse.cpp): that proves the builders
and the reference without a GPU and checks the host parser at the same edges.
"""
import functools
import os
import re

import numpy as np
import pytest
import torch

from fastapriori_amd.ops import _native
from fastapriori_amd.ops import primitives as prim
from fastapriori_amd.utils import io
from fastapriori_amd.utils.jvm import java_split_ws, split_lines

DEV = torch.device("cuda", 0)
gpu = pytest.mark.gpu

# csrc/hip/parse.hip: kLTile = kTTile, kLB = kTBy, kHalo, kSeenT / kSeen, kPT, and the
# 256-line chunk of k_tcompact (test_boundary_constants guards the tile size)
B = 16384          # tile
CH = 64            # thread chunk
HALO = 2048        # bytes staged in front of a tile
SEEN_T = 16        # LDS column of the numeric tile parser
SEEN_D = 64        # LDS column of the dictionary parser
DICT_BLK = 128     # lines per dictionary parse block
CCHUNK = 256       # lines per compaction chunk


# ---------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------
_NUM = re.compile(r"0|[1-9][0-9]*")
_M64 = (1 << 64) - 1


def _token_hash(t: bytes) -> int:
    """FNV-1a over the bytes, then the splitmix64 finaliser of h ^ length."""
    h = 0xCBF29CE484222325
    for c in t:
        h = ((h ^ c) * 0x100000001B3) & _M64
    z = ((h ^ len(t)) + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def _line_starts(data: bytes):
    """[(start offset, line)] of every line of the data (latin-1 text)."""
    text = data.decode("latin-1")
    out, pos = [], 0
    for ln in split_lines(text):
        out.append((pos, ln))
        pos += len(ln)
        if text[pos:pos + 2] == "\r\n":
            pos += 2
        elif pos < len(text):
            assert text[pos] in "\r\n"
            pos += 1
    assert pos == len(text)
    return out


class Ref:
    """Expected parse of the lines of ``data`` that start in [b, e)."""

    def __init__(self, data: bytes, b: int = 0, e: int | None = None):
        e = len(data) if e is None else e
        lines = [(s, ln) for s, ln in _line_starts(data) if b <= s < e]
        self.starts = [s for s, _ in lines]
        self.rows, self.extras = [], []
        for _, ln in lines:
            seen, row = set(), []
            for t in java_split_ws(ln):
                if t in seen:
                    self.extras.append(t)
                else:
                    seen.add(t)
                    row.append(t)
            self.rows.append(row)
        self.n_lines = len(self.rows)
        self.off = [0]
        for r in self.rows:
            self.off.append(self.off[-1] + len(r))
        flat = [t for r in self.rows for t in r]
        self.numeric = all(t == "" or (_NUM.fullmatch(t) is not None and int(t) <= 2 ** 31 - 2)
                           for t in flat + self.extras)
        self.flat_bytes = [t.encode("latin-1") for t in flat]
        self.extra_bytes = [t.encode("latin-1") for t in self.extras]
        self.n_tokens = len(set(self.flat_bytes))
        if self.numeric:
            self.items = [0 if t == "" else int(t) + 1 for t in flat]
            self.xids = [0 if t == "" else int(t) + 1 for t in self.extras]
            self.V = max(self.items) + 1 if self.items else 0
            self.hist = np.bincount(np.array(self.items + self.xids, np.int64), minlength=self.V) \
                if self.V <= 1 << 20 else None


@functools.lru_cache(maxsize=None)
def _ref(name):
    return Ref(CASES[name]())


# ---------------------------------------------------------------------------
# builders
# ---------------------------------------------------------------------------
_FILL_TAIL = {0: b"", 2: b"7\n", 3: b"78\n", 4: b"7 8\n", 5: b"7 89\n", 7: b"7 8 19\n"}


def _fill(n: int) -> bytes:
    """Exactly n bytes of short numeric lines, the last one terminated by '\\n'."""
    assert n == 0 or n >= 2, n
    q, t = ((n - 7) // 6, _FILL_TAIL[7]) if n % 6 == 1 else (n // 6, _FILL_TAIL[n % 6])
    out = b"".join(b"%d %d %d\n" % (1 + i % 3, 4 + i // 3 % 3, 7 + i // 9 % 3) for i in range(q)) + t
    assert len(out) == n and (n == 0 or out[-1:] == b"\n")
    return out


def _body(n: int, first: int = 1000, count: int = 7000) -> bytes:
    """A line body of exactly n >= 4 bytes: 4-digit tokens first, first + 1, .. (cycling
    after ``count`` of them: repeats), single blanks, the slack as blanks after token 0."""
    assert n >= 4 and 1000 <= first and first + count <= 10000
    k = (n + 1) // 5
    toks = [b"%d" % (first + i % count) for i in range(k)]
    out = toks[0] + b" " * (n - (5 * k - 1)) + (b" " + b" ".join(toks[1:]) if k > 1 else b"")
    assert len(out) == n and out[:1] != b" " and out[-1:] != b" "
    return out


def _ids_line(ids) -> bytes:
    return b" ".join(b"%d" % (i - 1) for i in ids) + b"\n"


def _terms(data: bytes):
    """Offsets of the line ends: '\\n', and '\\r' not followed by '\\n'."""
    return [i for i, c in enumerate(data)
            if c == 10 or (c == 13 and data[i + 1:i + 2] != b"\n")]


CASES = {}


def case(name):
    def deco(fn):
        assert name not in CASES
        CASES[name] = functools.lru_cache(maxsize=None)(fn)
        return fn
    return deco


# --- A. terminator placement ------------------------------------------------
def _a_term(term, pos):
    def build():
        head = _fill(pos - 5) + b"41 42"
        data = head + term + b"43 44\n" + _fill(70)
        assert data[pos:pos + len(term)] == term and data[pos - 1:pos] == b"2"
        assert data[pos + len(term):pos + len(term) + 1] == b"4"      # a digit follows
        return data
    return build


for _tn, _t in (("lf", b"\n"), ("cr", b"\r"), ("crlf", b"\r\n")):
    for _pn, _p in (("62", 62), ("63", 63), ("64", 64), ("B-2", B - 2), ("B-1", B - 1), ("B", B)):
        case(f"A_{_tn}_at_{_pn}")(_a_term(_t, _p))


@case("A_cr_is_last_byte")
def _():
    data = _fill(100) + b"41 42\r"
    assert data[-1:] == b"\r"
    return data


@case("A_cr_is_last_byte_at_tile_edge")
def _():
    data = _fill(B - 6) + b"41 42\r"
    assert len(data) == B and data[B - 1:] == b"\r"     # nothing staged behind it but the pad
    return data


@case("A_cr_cr_lf_over_tile_edge")
def _():
    data = _fill(B - 7) + b"41 42\r\r\n43\n" + _fill(60)
    assert data[B - 2:B + 1] == b"\r\r\n"
    return data


@case("A_cr_cr_lf_over_chunk_edge")
def _():
    data = _fill(57) + b"41 42\r\r\n43\n" + _fill(60)
    assert data[62:65] == b"\r\r\n"
    return data


@case("A_chunk_of_64_newlines")
def _():
    data = _fill(64) + b"\n" * 64 + b"5 6\n"
    assert data[64:128] == b"\n" * 64 and data[63:64] == b"\n" and data[128:129] == b"5"
    return data


@case("A_last_chunk_of_tile_all_newlines")
def _():
    data = _fill(B - 64) + b"\n" * 64 + b"5 6\n" + _fill(40)
    assert data[B - 64:B] == b"\n" * 64 and data[B:B + 1] == b"5"
    return data


# --- B. line start against the halo ------------------------------------------
def _halo_line(d, P=0):
    """A line that ends in the first chunk of tile 1 (of the region starting at P) and
    starts at that tile's start - HALO + d."""
    T1 = (P & ~63) + B
    S = T1 - HALO + d
    data = _fill(P) + _fill(S - P) + _body(T1 + 10 - S) + b"\n" + _fill(200)
    assert data[S - 1:S] == b"\n" and data[T1 + 10:T1 + 11] == b"\n"
    assert not [i for i in _terms(data) if S <= i < T1 + 10]
    assert P == 0 or data[P - 1:P] == b"\n"
    return data


for _d in (-1, 0, 1):
    case(f"B_line_start_at_halo{_d:+d}")(functools.partial(_halo_line, _d))
    case(f"B_region65_line_start_at_halo{_d:+d}")(functools.partial(_halo_line, _d, 65))


def _halo_tokens():
    L0 = B - HALO
    S = L0 - 98
    seg = b"".join(b"%d " % v for v in range(10, 42))                # 96 bytes of 2-digit tokens
    mid = _body(B - 3 - (L0 + 4) - 2, 2000)
    data = _fill(S) + seg + b"123456 " + mid + b" 7654321 55\n" + _fill(100)
    return data, L0


@case("B_tokens_straddle_halo_start_and_tile_edge")
def _():
    data, L0 = _halo_tokens()
    assert data[L0 - 2:L0 + 4] == b"123456" and data[L0 - 3:L0 - 2] == b" "     # HBM dwords -> LDS dwords
    assert data[B - 3:B + 4] == b"7654321" and data[B + 4:B + 8] == b" 55\n"
    assert not [i for i in _terms(data) if L0 - 98 <= i < B + 7]
    return data


@case("B_line_longer_than_two_tiles")
def _():
    data = _fill(100) + _body(2 * B + 3000, 1000, 300) + b"\n5 6\n" + _fill(300)
    t = _terms(data)
    assert not [i for i in t if B <= i < 2 * B]                      # tile 1 holds no line end
    assert data[100 + 2 * B + 3000:][:5] == b"\n5 6\n" and len(data) <= 3 * B + 1024
    return data


# --- D. tail line --------------------------------------------------------------
@case("D_tail_ends_at_chunk_edge")
def _():
    data = _fill(123) + b"41 42"
    assert len(data) == 2 * CH
    return data


@case("D_tail_ends_at_tile_edge")
def _():
    data = _fill(B - 5) + b"41 42"
    assert len(data) == B
    return data


@case("D_tail_starts_at_tile_edge")
def _():
    data = _fill(B) + b"41 42"
    assert data[B - 1:B + 1] == b"\n4"
    return data


@case("D_tail_with_trailing_blanks")
def _():
    data = _fill(60) + b"41 42  \t \x0b"
    assert data[59:65] == b"\n41 42" and not data[65:].strip(b" \t\x0b")      # the tail crosses the chunk edge
    return data


@case("D_tail_is_whitespace_only")
def _():
    data = _fill(50) + b"  \t "
    assert data[49:50] == b"\n" and len(data) < CH and not data[50:].strip()
    return data


@case("D_tail_is_whitespace_only_over_chunk_edge")
def _():
    data = _fill(62) + b"    "
    assert data[61:62] == b"\n" and len(data) == 66
    return data


@case("D_tail_longer_than_halo")
def _():
    data = _fill(B - 3000) + _body(4000)
    assert _terms(data)[-1] == B - 3001 and len(data) == B + 1000
    return data


@case("D_single_tail_token")
def _():
    return b"5"


@case("D_single_newline")
def _():
    return b"\n"


# --- E. lines per tile ----------------------------------------------------------
@case("E_tile_of_newlines")
def _():
    data = b"\n" * B + b"5 6\n"
    assert data[:B] == b"\n" * B
    return data


@case("E_8192_one_token_lines")
def _():
    data = b"1\n" * 8192
    assert len(data) == B
    return data


def _n_lines(n, tail):
    def build():
        data = b"".join(b"%d %d\n" % (10 + i % 7, 20 + i % 11) for i in range(n)) + (b"3 4" if tail else b"")
        assert len(_terms(data)) == n and len(data) < B
        return data
    return build


for _n in (CCHUNK - 1, CCHUNK, CCHUNK + 1):
    case(f"E_{_n}_lines_in_one_tile")(_n_lines(_n, False))
    case(f"E_{_n}_lines_and_a_tail")(_n_lines(_n, True))


def _wide_line(n):
    def build():
        data = _fill(40) + _ids_line(range(1001, 1001 + n)) + b"5 6\n"
        assert len(set(data.split(b"\n")[-3].split())) == n
        return data
    return build


for _n in (255, 256, 257):
    case(f"E_line_of_{_n}_ids")(_wide_line(_n))


# --- F. bad tokens, and their accepted neighbours, inside one 64-byte chunk -------
BAD_TOKENS = {"2147483647": b"2147483647", "4294967296": b"4294967296", "9999999999": b"9999999999",
              "10000000000": b"10000000000", "00": b"00", "01": b"01", "minus1": b"-1", "plus1": b"+1",
              "1.0": b"1.0", "nul": b"4\x005", "x01": b"4\x015", "xe9": b"4\xe95"}
GOOD_LINES = {"0": b"1 0", "2147483646": b"1 2147483646", "vt_ff_separators": b"4\x0b5\x0c6",
              "controls_at_line_ends": b"\x01\x00 5 \x02\x00"}


def _chunk_lines(tok, where, tile):
    """The four lines that end inside the chunk [c0, c0 + 64); the line ``tok`` is line ``where``."""
    def build():
        c0 = tile * B + 2 * CH
        lines = [b"2 3\n", b"4 5\n", b"6 7\n", b"8 9\n"]
        lines[where] = tok + b"\n"
        data = _fill(c0) + b"".join(lines) + _body(CH) + b"\n" + _fill(120) + b"11 12"
        ends = [i for i in _terms(data) if c0 <= i < c0 + CH]
        assert len(ends) == 4 and data[c0 - 1:c0] == b"\n"
        s = c0 + sum(len(x) for x in lines[:where])
        assert data[s:s + len(tok) + 1] == tok + b"\n"
        return data
    return build


for _tile in (0, 1):
    for _wn, _w in (("first", 0), ("middle", 1), ("last", 3)):
        for _k, _tok in BAD_TOKENS.items():
            case(f"F_bad_{_k}_{_wn}_line_tile{_tile}")(_chunk_lines(b"1 " + _tok, _w, _tile))
    for _k, _tok in GOOD_LINES.items():
        case(f"F_good_{_k}_tile{_tile}")(_chunk_lines(_tok, 1, _tile))


# --- G. duplicates ----------------------------------------------------------------
def _filter_bits(i):
    return ((i * 0x9E3779B1) & 0xFFFFFFFF) >> 25


def _repeat_line(n, pos):
    def build():
        ids = list(range(101, 101 + n))
        data = _fill(30) + _ids_line(ids + [ids[pos]]) + b"5 6\n"
        assert len(set(ids)) == n and pos < n
        return data
    return build


assert SEEN_T == 16      # positions 0 .. 15 sit in the LDS column, 16 on in scratch
for _n, _pos in ((15, 0), (15, 14), (16, 0), (16, 15), (17, 0), (17, 15), (17, 16)):
    case(f"G_{_n}_ids_then_repeat_of_position_{_pos}")(_repeat_line(_n, _pos))


def _colliding(i, lo=1, hi=4000):
    return next(j for j in range(lo, hi) if j != i and _filter_bits(j) == _filter_bits(i))


@case("G_filter_hit_is_not_a_duplicate")
def _():
    a = 11
    b = _colliding(a)
    ids = list(range(501, 518))                              # 17 distinct: position 16 is in scratch
    c0, c16 = _colliding(ids[0], 600), _colliding(ids[16], 600)
    assert a != b and _filter_bits(a) == _filter_bits(b)
    assert c0 not in ids and c16 not in ids and _filter_bits(c0) == _filter_bits(ids[0]) \
        and _filter_bits(c16) == _filter_bits(ids[16])
    return _ids_line([a, b]) + _ids_line(ids + [c0, c16]) + _ids_line([a, b, a, b])


@case("G_more_ids_than_filter_bits")
def _():
    ids = list(range(1001, 1201))                            # 200 distinct > 128 filter bits
    new = list(range(2001, 2021))
    rep = [ids[0], ids[15], ids[16], ids[130], new[3], ids[199]]
    return _fill(20) + _ids_line(ids + new + rep) + b"5 6\n"


@case("G_one_id_four_times")
def _():
    return b"3 3 3 3\n"


@case("G_repeats_in_a_line_longer_than_halo")
def _():
    data = _fill(B - 3000) + _body(4000, 1000, 300) + b"\n5 5\n"
    assert _terms(data)[-2] == B + 1000                      # starts before the halo, ends in tile 1
    return data


# --- H. histogram -----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _hist_cap():
    return prim.limits().kHistCap


@case("H_largest_id_in_histogram")
def _():
    return b"1 2 2\n%d 2 %d\n" % (_hist_cap() - 2, _hist_cap() - 2)


@case("H_first_id_past_histogram")
def _():
    return b"1 2 2\n%d 2 %d\n" % (_hist_cap() - 1, _hist_cap() - 1)


# --- dictionary path ----------------------------------------------------------------
def _wfill(n):
    """Exactly n bytes of short word lines ending in '\\n'."""
    return _fill(n).replace(b"7", b"w").replace(b"8", b"x")


def _dict_term(term, pos):
    def build():
        data = _wfill(pos - 5) + b"ab cd" + term + b"ef gh\n" + _wfill(70)
        assert data[pos:pos + len(term)] == term and data[pos + len(term):][:1] == b"e"
        return data
    return build


for _tn, _t in (("lf", b"\n"), ("cr", b"\r"), ("crlf", b"\r\n")):
    for _pn, _p in (("63", 63), ("64", 64), ("B-1", B - 1), ("B", B)):
        case(f"dict_{_tn}_at_{_pn}")(_dict_term(_t, _p))


def _dict_lines(n):
    def build():
        data = b"".join(b"w%d v%d\n" % (i % 50, i % 7) for i in range(n))
        assert len(_terms(data)) == n
        return data
    return build


for _n in (DICT_BLK - 1, DICT_BLK, DICT_BLK + 1):
    case(f"dict_{_n}_lines")(_dict_lines(_n))


def _dict_wide(n):
    def build():
        toks = [b"t%d" % i for i in range(n)]
        rep = [toks[p] for p in (0, SEEN_D - 1, SEEN_D) if p < n]
        assert len(set(toks)) == n
        return b"a b\n" + b" ".join(toks + rep) + b"\nc\n"
    return build


for _n in (SEEN_D - 1, SEEN_D, SEEN_D + 1):
    case(f"dict_line_of_{_n}_tokens_then_repeats")(_dict_wide(_n))


@case("dict_blank_lines_and_blank_tail")
def _():
    return b"a\n\n  \t\nb a\n\r\n\n \t"


@case("dict_blank_lines_terminated")
def _():
    return b"\n\na\n\n"


@case("dict_tokens_differ_in_length_or_last_byte")
def _():
    return b"ab abc abd ab a abcd abc\nabd ab\x01 ab\x02\n"


@case("dict_high_bytes")
def _():
    return b"\xe9 \xe9\xe9 \xff\x80 \xe9\n\xa0 \x85 caf\xc3\xa9 \xa0\n"


NUMERIC_CASES = [k for k in CASES if not k.startswith("dict_")]
DICT_CASES = [k for k in CASES if k.startswith("dict_") or k.startswith("F_bad_")]


# ---------------------------------------------------------------------------
# comparisons
# ---------------------------------------------------------------------------
def _last_is_term(data):
    return data[-1:] in (b"\n", b"\r")


def _check_host(sh, ref):
    assert sh.vocab.numeric == ref.numeric
    assert sh.offsets.tolist() == ref.off
    if ref.numeric:
        assert sh.items.tolist() == ref.items
        assert sh.extras.tolist() == ref.xids
        assert sh.vocab.size == ref.V
        return
    so, blob = sh.vocab.offsets, sh.vocab.blob.tobytes()
    tok = [blob[int(so[i]):int(so[i + 1])] for i in range(sh.vocab.size)]
    assert [tok[i] for i in sh.items.tolist()] == ref.flat_bytes
    assert [tok[i] for i in sh.extras.tolist()] == ref.extra_bytes
    assert len(tok) == ref.n_tokens == len(set(tok))
    assert sh.vocab.hashes.tolist() == [_token_hash(t) for t in tok]


def _dev_buf(data):
    n = len(data)
    host = torch.zeros((n + 63) // 64 * 64 + 64, dtype=torch.uint8)
    host[:n] = torch.frombuffer(bytearray(data), dtype=torch.uint8)
    return host.to(DEV)


def _check_numeric(got, ref):
    assert ref.numeric and got is not None and not isinstance(got, int)
    off, items, extras, V, hist = got
    assert off.tolist() == ref.off
    assert items.tolist() == ref.items
    assert extras.tolist() == ref.xids
    assert V == ref.V
    assert (hist is None) == (ref.V > _hist_cap())
    if hist is not None:
        assert hist.tolist() == ref.hist.tolist()


def _check_dict(got, ref, data, base=0):
    assert got is not None
    off, items, extras, hashes, pos, lens = got
    tok = [data[base + p:base + p + n] for p, n in zip(pos.tolist(), lens.tolist())]
    assert off.tolist() == ref.off
    assert [tok[i] for i in items.tolist()] == ref.flat_bytes
    assert [tok[i] for i in extras.tolist()] == ref.extra_bytes
    assert len(tok) == ref.n_tokens == len(set(tok))
    assert hashes.tolist() == [_token_hash(t) for t in tok]


def _tile_parse(data, cuts=(), n_lines="device", xcap=None, fill=None, icap=None):
    """TileParse over the regions [0, c1), [c1, c2), .. of the data; n_lines: "device"
    (None: read back), "host" (given) or "mixed" (alternating)."""
    n, starts = len(data), [s for s, _ in _line_starts(data)]
    buf = _dev_buf(data)
    tp = prim.TileParse(buf, n, DEV, n, xcap, icap)
    if fill is not None:
        tp.items.fill_(fill)
    edges = [0] + list(cuts) + [n]
    assert all(c in starts for c in edges[:-1]) and edges == sorted(set(edges))
    for k, (lo, hi) in enumerate(zip(edges[:-1], edges[1:])):
        given = n_lines == "host" or (n_lines == "mixed" and k % 2 == 0)
        nl = sum(lo <= s < hi for s in starts) if given else None
        tp.region(lo, hi, nl, tail=hi == n and not _last_is_term(data))
    return tp, tp.finish()


# ---------------------------------------------------------------------------
# host parser against the reference (no GPU): builders, reference, parse.cpp
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_host_parser(name):
    _check_host(io.parse_bytes(CASES[name]()), _ref(name))


def test_cases_are_small_and_decided_as_named():
    for name in CASES:
        assert len(CASES[name]()) <= 3 * B + 1024, name
        assert _ref(name).numeric == (name not in DICT_CASES), name


RANGE_CASES = [("A_crlf_at_B-1", B - 1, B), ("A_crlf_at_B-1", B, B + 2), ("A_crlf_at_B-1", B + 1, 10 ** 9),
               ("A_crlf_at_B-1", 0, B), ("A_cr_at_B-1", B, B + 40), ("A_lf_at_63", 64, 65),
               ("B_line_start_at_halo+0", B - HALO, B), ("B_line_start_at_halo+0", B - HALO + 1, 10 ** 9),
               ("D_tail_longer_than_halo", B - 3000, B), ("F_bad_01_middle_line_tile1", B, 10 ** 9),
               ("F_bad_01_middle_line_tile1", 0, B),
               ("E_tile_of_newlines", 0, 10 ** 9), ("E_tile_of_newlines", B - 1, 10 ** 9)]


@pytest.mark.parametrize("name,b,e", RANGE_CASES)
def test_host_parser_byte_ranges(tmp_path, name, b, e):
    data = CASES[name]()
    p = tmp_path / "D.dat"
    p.write_bytes(data)
    _check_host(io.parse_file(str(p), b, min(e, len(data))), Ref(data, b, e))


def test_reference_on_known_lines():
    r = Ref(b"1 2 1\r\n\r 07\n0 2147483646")
    assert r.rows == [["1", "2"], [""], ["07"], ["0", "2147483646"]] and r.extras == ["1"] and not r.numeric
    r = Ref(b"1 2 1\r\n\r7\n0 2147483646", 1, 8)
    assert r.starts == [7] and r.numeric and r.items == [0] and r.V == 1
    assert Ref(b"2147483647\n").numeric is False and Ref(b"").V == 0


# ---------------------------------------------------------------------------
# device parser against the reference
# ---------------------------------------------------------------------------
@gpu
def test_boundary_constants():
    lib = _native.hip()
    assert lib.fa_hip_parse_tiles(B) == 1 and lib.fa_hip_parse_tiles(B + 1) == 2
    assert lib.fa_hip_tparse_tiles(63, 64 + B) == 2
    assert _hist_cap() > 256


@gpu
@pytest.mark.parametrize("name", NUMERIC_CASES)
def test_numeric_tile_parser(name):
    """parse_numeric_device on the whole buffer; a not-numeric input must come back as
    None and then parse in dictionary mode to the reference."""
    data, ref = CASES[name](), _ref(name)
    got = prim.parse_numeric_device(_dev_buf(data), len(data), _last_is_term(data))
    if ref.numeric:
        _check_numeric(got, ref)
    else:
        assert got is None
        _check_dict(prim.parse_dict_device(_dev_buf(data), len(data), _last_is_term(data)), ref, data)


@gpu
@pytest.mark.parametrize("name", [k for k in CASES if k.startswith("dict_")])
def test_dictionary_parser(name):
    data, ref = CASES[name](), _ref(name)
    assert prim.parse_numeric_device(_dev_buf(data), len(data), _last_is_term(data)) is None
    _check_dict(prim.parse_dict_device(_dev_buf(data), len(data), _last_is_term(data)), ref, data)


# --- C. regions ----------------------------------------------------------------------
def _region_cuts():
    """Three tiles of lines with line starts placed at lo % 64 = 0, 1, 63, just past a
    tile edge, and at a region end that makes hi - (lo & ~63) a multiple of the tile."""
    want = [5 * CH, 9 * CH + 1, 20 * CH + 63, B + 1, 5 * CH + B, 2 * B + CH + 63, 3 * B - 80]
    data, cuts = b"", []
    for w in want:
        data += _fill(w - len(data))
        cuts.append(len(data))
    data += _fill(40) + b"41 42"
    assert cuts == want and [c % 64 for c in cuts[:3]] == [0, 1, 63] and cuts[3] == B + 1
    assert cuts[4] - (cuts[0] & ~63) == B
    assert all(data[c - 1:c] == b"\n" for c in cuts) and len(data) == 3 * B - 35
    return data, cuts


REGION_CASES = {
    "three_tiles_mixed_lo": lambda: _region_cuts(),
    # hi - (lo & ~63) = B exactly, then a region that is one tile and a tail
    "multiple_of_tile_no_tail": lambda: (_region_cuts()[0], [5 * CH, 5 * CH + B]),
    "halo_reaches_before_lo-1": lambda: (_halo_line(-1, 65), [65]),
    "halo_reaches_before_lo+0": lambda: (_halo_line(0, 65), [65]),
    "halo_reaches_before_lo+1": lambda: (_halo_line(1, 65), [65]),
    "halo_line_starts_region": lambda: (_halo_line(0, 0), [B - HALO]),
    "one_byte_region": lambda: (b"1 2\n\n3\n", [4, 5]),
    "tail_only_region": lambda: (b"1 2\n5", [4]),
    "crlf_split_over_tile_edge": lambda: (CASES["A_crlf_at_B-1"](), [B + 1]),
    "bad_token_in_second_region": lambda: (CASES["F_bad_01_first_line_tile1"](), [B + 2 * CH]),
    "bad_token_in_first_region": lambda: (CASES["F_bad_01_first_line_tile0"](),
                                          [_terms(CASES["F_bad_01_first_line_tile0"]())[-1] + 1]),
}


def test_region_builders():
    for name, fn in REGION_CASES.items():
        data, cuts = fn()
        starts = [s for s, _ in _line_starts(data)]
        assert all(c in starts for c in cuts), name


@gpu
@pytest.mark.parametrize("n_lines", ["device", "host", "mixed"])
@pytest.mark.parametrize("name", list(REGION_CASES))
def test_regions(name, n_lines):
    data, cuts = REGION_CASES[name]()
    ref = Ref(data)
    _, got = _tile_parse(data, cuts, n_lines)
    if ref.numeric:
        _check_numeric(got, ref)
    else:
        assert got is None


@gpu
def test_region_ending_a_tile_multiple_with_tail():
    data = _fill(65) + _fill(B - 6) + b"41 42"
    assert len(data) - 64 == B and data[64:65] == b"\n"
    _, got = _tile_parse(data, [65])
    _check_numeric(got, Ref(data))


@gpu
@pytest.mark.parametrize("n_lines", ["device", "mixed"])
def test_one_region_per_line(n_lines):
    data = CASES["A_chunk_of_64_newlines"]() + b"1 1 2\r\n3\r4 4\n" + _fill(200) + b"9 9"
    starts = [s for s, _ in _line_starts(data)]
    assert len(starts) > 100
    ref = Ref(data)
    assert len(ref.items) > (len(data) + 1) // 2 + 1          # blank lines: one id per byte
    _, got = _tile_parse(data, starts[1:], n_lines, icap=len(ref.items))
    _check_numeric(got, ref)


@gpu
@pytest.mark.parametrize("grid", [1, 3])
def test_compaction_grid(monkeypatch, grid):
    # three tiles on one or three workgroups: the tile stride loop, one histogram row each
    monkeypatch.setattr(prim.TileParse, "GRID", grid)
    data, cuts = _region_cuts()
    assert int(_native.hip().fa_hip_tparse_tiles(0, len(data))) == 3 >= grid
    for c in ([], cuts[3:5]):
        _, got = _tile_parse(data, c)
        _check_numeric(got, Ref(data))


# --- F. the compaction stays off a bad parse ------------------------------------------
@gpu
@pytest.mark.parametrize("name", ["F_bad_01_first_line_tile0", "F_bad_xe9_middle_line_tile1"])
def test_bad_parse_leaves_items_untouched(name):
    """k_tparse leaves a thread's line loop at its first bad token, so the later lines of
    that thread have no counts; k_tcompact must not run on them.  Any compaction at all
    would store the ids of the other threads' lines over the sentinel."""
    data = CASES[name]()
    tp, got = _tile_parse(data, fill=-7)
    assert got is None
    assert bool((tp.items == -7).all())
    assert tp.hpart.count_nonzero().item() == 0


# --- E. more ids than (bytes + 1) / 2 --------------------------------------------------
@gpu
def test_blank_lines_overflow_items_and_parse_again():
    data = CASES["E_tile_of_newlines"]()
    tp, got = _tile_parse(data, fill=-7)
    assert got == 0 and tp.need_items == B + 2 > tp.icap       # no repeats; every id counted
    assert bool((tp.items == -7).all())


# --- H. repeat buffer ---------------------------------------------------------------------
@gpu
def test_repeat_buffer_capacity():
    data = _fill(B - 20) + b"1 1 1 2 2\n" * 9 + b"3 3"
    ref = Ref(data)
    R = len(ref.xids)
    assert R == 28
    _, got = _tile_parse(data, xcap=R)
    _check_numeric(got, ref)
    _, got = _tile_parse(data, xcap=R - 1)
    assert isinstance(got, int) and got == R


# --- byte ranges through the file reader ------------------------------------------------------
@gpu
@pytest.mark.parametrize("name,b,e", RANGE_CASES)
def test_file_byte_ranges(tmp_path, name, b, e):
    data = CASES[name]()
    p = os.path.join(tmp_path, "D.dat")
    with open(p, "wb") as f:
        f.write(data)
    ref = Ref(data, b, e)
    got = io.parse_file_device(p, b, min(e, len(data)), DEV)
    assert got is not None and got.vocab.numeric == ref.numeric
    if ref.numeric:
        _check_numeric((got.offsets, got.items, torch.from_numpy(got.extras), got.vocab.size, got.hist), ref)
    else:
        _, first, pos, lens = got.vocab.file_src
        _check_dict((got.offsets, got.items, torch.from_numpy(got.extras), got.vocab.hashes, pos, lens),
                    ref, data, first)
