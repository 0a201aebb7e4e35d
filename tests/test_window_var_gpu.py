"""Window encode on windows of their own length (fecgpu_rlc_window_encode_rows_var_host) against the CPU
oracle: window w is Oracle.rlc_encode_block(0, stream[wrow[w] : wrow[w] + wlen[w]], r) on the rows truncated
to blk_len[w] and zero-padded to it.  Byte work: every comparison is exact.  The cases are those of
test_window_rows_gpu.py with a length per window: ragged rows at 4-byte aligned, never 16-byte aligned
offsets of one pool, 0xA5 canaries between them, and after each call the whole pool image is compared with
the expected one: stream rows untouched, every repair row exactly blk_len[w] bytes, canaries intact.

The shapes are the smallest at which the chunks of the length classes can go wrong: width 48 (42 windows per
chunk, so a class boundary falls where a plain chunk would continue), 1200, 2064 (a window over two chunks);
every class a single window; a class that fills whole chunks exactly before the next; a class ending in a
partial chunk before the next; shuffled lengths over runs out of order with a gap and a repeated window; a
window of length 1; kmax 128 with one window of 128 among windows of 1; r 1, 2, 5, 8 (every tile width) and 11
(a second tile)."""
import numpy as np
import pytest

import test_window_rows_gpu as WR
import test_xor_rows_gpu as XR
from oracle_py import Oracle

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def eng():
    from pquic_amd import Engine
    if not torch.cuda.is_available():
        pytest.fail("GPU test run without a visible GPU")
    return Engine(0)


@pytest.fixture(scope="module")
def oracle():
    return Oracle()


@pytest.fixture(scope="module")
def hostpath(eng):
    from pquic_amd.engine import HostPath
    hp = HostPath(0, nstreams=3, chunk_bytes=64 << 10)
    yield hp
    hp.close()


def windows(kind, kmax, nwin, rng):
    """(wrow, wlen) of a length pattern."""
    if kind == "alldiff":      # every class is one window: kmax windows, every length once, shuffled
        wlen = rng.permutation(np.arange(1, kmax + 1))
        return list(range(len(wlen))), wlen
    if kind == "whole":        # 128 windows of 4 rows (3 whole chunks at width 48), then a class of 9 around them
        wlen = [9] * 5 + [4] * 128 + [9] * (nwin - 133)
        return WR.starts("overlap", kmax, nwin), wlen
    if kind == "partial":      # 100 windows of 5 rows end in a partial chunk at every width; 12 and 30 follow
        wlen = [5, 12] * 100 + [30] * (nwin - 200)
        return WR.starts("overlap", kmax, nwin), wlen
    if kind == "mixed":        # runs out of order, a gap, a repeated window; shuffled lengths, some of 1 and of kmax
        wlen = rng.integers(1, kmax + 1, nwin)
        wlen[[0, nwin // 2]] = 1
        wlen[[1, nwin - 1]] = kmax
        return WR.starts("mixed", kmax, nwin), wlen
    if kind == "one128":       # kmax 128: one window of 128 rows, the rest of 1
        wlen = np.ones(nwin, np.int64)
        wlen[nwin // 3] = 128
        return WR.starts("overlap", kmax, nwin), wlen
    assert kind == "equal"     # every window kmax long: the call is the plain rows form
    return WR.starts("mixed", kmax, nwin), [kmax] * nwin


class VarCase(WR.Case):
    """WR.Case with a length per window: the same pool, row lengths, window lengths in bytes and tables."""

    def __init__(self, oracle, S, kmax, r, kind, nwin, seed):
        rng = np.random.default_rng(seed)
        wrow, wlen = windows(kind, kmax, nwin, rng)
        self.S, self.k, self.r, self.nwin = S, kmax, r, len(wrow)
        nwin = self.nwin
        self.wrow, self.wlen = np.array(wrow, np.uint32), np.array(wlen, np.uint8)
        self.nrows = nrows = int((self.wrow + self.wlen).max())
        cand = sorted({min(max(x, 0), S) for x in (0, 1, 3, 4, 15, 16, 17, S - 1, S)})
        lens = [cand[x % len(cand)] if rng.random() < 0.4 else int(rng.integers(0, S + 1)) for x in range(nrows)]
        if nrows >= 3:
            lens[nrows - 1] = 0      # a row of 0 bytes: its address is 0
        lens[int(self.wrow[0])] = S  # window 0 holds a full row
        bcand = sorted({min(max(x, 1), S) for x in (1, 3, 4, 15, 16, 17, S - 1, S)})
        blk = []
        for w in range(nwin):
            ws, wl = int(self.wrow[w]), int(self.wlen[w])
            if w % 3 == 0:
                blk.append(max(lens[ws:ws + wl]))           # the reference's max_length (0: nothing is written)
            else:
                blk.append(bcand[(w // 3) % len(bcand)])    # any length: longer rows are truncated for this window
        if nwin > 1:
            blk[1] = max(1, S // 2 - 1)                     # window 1: shorter than a row it holds
            lens[int(self.wrow[1])] = S
        p = XR.Pool()
        self.row_off = [p.add(n) if n else None for n in lens]
        self.rep_off = [p.add(blk[w]) if blk[w] else None for w in range(nwin) for _ in range(r)]
        self.row_len = np.array(lens, np.uint32)
        self.blk_len = np.array(blk, np.uint32)
        self.image = p.image()
        self.rows = []
        for x in range(nrows):
            d = rng.integers(0, 256, lens[x], dtype=np.uint8)
            if lens[x]:
                self.image[self.row_off[x]:self.row_off[x] + lens[x]] = d
            self.rows.append(d)
        self.want = self.image.copy()
        for w in range(nwin):
            bl, ws, wl = blk[w], int(self.wrow[w]), int(self.wlen[w])
            if not bl:
                continue
            srcs = [self.rows[x][:bl] for x in range(ws, ws + wl)]
            if max(len(s) for s in srcs) < bl:  # zero-padding to the window's length changes no repair byte
                srcs[0] = np.concatenate([srcs[0], np.zeros(bl - len(srcs[0]), np.uint8)])
            ret, reps = oracle.rlc_encode_block(0, srcs, r)
            assert ret == 0 and len(reps) == r and all(len(x) == bl for x in reps)
            for i in range(r):
                o = self.rep_off[w * r + i]
                self.want[o:o + bl] = reps[i]

    def tables(self, base):
        t = super().tables(base)
        t["wlen"] = self.wlen
        return t


# S, kmax, r, length pattern, nwin
SHAPES = [
    (48, 30, 1, "alldiff", 30),
    (48, 30, 2, "whole", 150),      # the second class begins on a chunk with no padding
    (48, 30, 5, "partial", 300),
    (48, 30, 8, "mixed", 203),
    (44, 30, 11, "mixed", 100),     # symbol_size below the width of 48; a tile of 8 and a remainder
    (1200, 30, 2, "alldiff", 30),
    (1200, 30, 5, "mixed", 67),
    (1200, 30, 11, "partial", 210),
    (1200, 30, 8, "whole", 140),
    (2064, 30, 1, "mixed", 41),     # a window spans chunks
    (2064, 30, 8, "alldiff", 30),
    (2064, 30, 5, "partial", 201),
    (48, 128, 5, "one128", 90),
    (1200, 128, 2, "one128", 19),
]

_cases = {}


def case(oracle, *shape):
    """One reference per shape, shared by the tests and never modified."""
    if shape not in _cases:
        S, kmax, r, kind, nwin = shape
        _cases[shape] = VarCase(oracle, S, kmax, r, kind, nwin, 17 * S + 5 * kmax + r + nwin)
    return _cases[shape]


def run_host(eng, hostpath, c, pinned=True, pageable=(), var=True):
    """The host form on fresh buffers: rows in fecgpu_host_alloc memory, the tables page-locked or pageable."""
    lib = eng.lib
    hm = XR.HostMem(lib, True)
    try:
        pool = hm.array(c.image)
        t = {n: hm.array(v, pinned=pinned and n not in pageable) for n, v in c.tables(XR._dev_addr(lib, pool)).items()}
        if var:
            hostpath.rlc_window_encode_rows_var(t["rows"], t["row_len"], c.nrows, t["wrow"], t["wlen"], t["rep_rows"],
                                                t["blk_len"], c.nwin, c.k, c.r, c.S)
        else:
            hostpath.rlc_window_encode_rows(t["rows"], t["row_len"], c.nrows, t["wrow"], t["rep_rows"], t["blk_len"],
                                            c.nwin, c.k, c.r, c.S)
        return pool.copy()
    finally:
        hm.close()


@pytest.mark.parametrize("S,kmax,r,kind,nwin", SHAPES)
def test_matches_the_oracle(eng, oracle, hostpath, S, kmax, r, kind, nwin):
    c = case(oracle, S, kmax, r, kind, nwin)
    assert c.nwin <= 300
    assert any(o is None for o in c.row_off), "the case holds a row of 0 bytes at address 0"
    assert any(int(c.row_len[x]) > int(c.blk_len[w]) for w in range(c.nwin)
               for x in range(int(c.wrow[w]), int(c.wrow[w]) + int(c.wlen[w]))), "a row longer than one of its windows"
    got = run_host(eng, hostpath, c)
    bad = np.flatnonzero(got != c.want)
    assert not len(bad), (S, kmax, r, kind, nwin, bad[:8])


def test_the_patterns_are_what_they_claim(oracle):
    """The class tables of three cases: single-window classes, a class of whole chunks, a partial chunk."""
    from pquic_amd.engine import window_classes
    c = case(oracle, 48, 30, 1, "alldiff", 30)
    _, first, cnt, lens, cchunk, nch = window_classes(c.wlen, 30, 48)
    assert list(cnt) == [1] * 30 and list(lens) == list(range(1, 31)) and nch == 30
    c = case(oracle, 48, 30, 2, "whole", 150)
    _, first, cnt, lens, cchunk, nch = window_classes(c.wlen, 30, 48)
    assert list(cnt) == [128, 22] and list(cchunk) == [0, 3] and 128 * 48 == 3 * 2048
    c = case(oracle, 1200, 30, 11, "partial", 210)
    _, first, cnt, lens, cchunk, nch = window_classes(c.wlen, 30, 1200)
    assert list(lens) == [5, 12, 30] and (100 * 1200) % 2048 and list(cchunk) == [0, 59, 118]


@pytest.mark.parametrize("S,kmax,r,kind,nwin", [(48, 30, 8, "mixed", 203), (1200, 30, 5, "mixed", 67),
                                                (2064, 30, 5, "partial", 201)])
@pytest.mark.parametrize("mode", ["pageable", "one_pageable", "wlen_pageable"])
def test_tables_in_pageable_memory(eng, oracle, hostpath, mode, S, kmax, r, kind, nwin):
    c = case(oracle, S, kmax, r, kind, nwin)
    pageable = {"pageable": (), "one_pageable": ("blk_len",), "wlen_pageable": ("wlen",)}[mode]
    got = run_host(eng, hostpath, c, pinned=mode != "pageable", pageable=pageable)
    bad = np.flatnonzero(got != c.want)
    assert not len(bad), (mode, bad[:8])


@pytest.mark.parametrize("S,r", [(48, 2), (1200, 11), (2064, 5)])
def test_equal_lengths_are_the_plain_rows_form(eng, oracle, hostpath, S, r):
    """every wlen[w] == kmax: byte for byte HostPath.rlc_window_encode_rows on the same pool, and the oracle's"""
    c = case(oracle, S, 30, r, "equal", 60)
    assert set(c.wlen.tolist()) == {30}
    got = run_host(eng, hostpath, c)
    plain = run_host(eng, hostpath, c, var=False)
    assert np.array_equal(got, plain)
    assert np.array_equal(got, c.want), np.flatnonzero(got != c.want)[:8]


@pytest.mark.parametrize("S,kmax,r,kind,nwin", [(48, 30, 5, "partial", 300), (1200, 30, 5, "mixed", 67),
                                                (1200, 128, 2, "one128", 19)])
def test_block_path_with_padding_rows_gives_the_same_image(eng, oracle, hostpath, S, kmax, r, kind, nwin):
    """knob window_sc 0: every window a block of kmax rows, the positions past its length rows of 0 bytes"""
    c = case(oracle, S, kmax, r, kind, nwin)
    old = eng.get_knob("window_sc")
    try:
        eng.set_knob("window_sc", 0)
        got = run_host(eng, hostpath, c)
    finally:
        eng.set_knob("window_sc", old)
    bad = np.flatnonzero(got != c.want)
    assert not len(bad), bad[:8]
