"""Window jobs on rows (fecgpu_rlc_window_encode_rows and its host form) against the CPU oracle: window w
is Oracle.rlc_encode_block(0, stream[wrow[w] : wrow[w] + k], r) on the rows truncated to blk_len[w] and
zero-padded to it.  Byte work: every comparison is exact.  Stream rows and repair rows live in one pool at
4-byte aligned offsets that are never 16-byte aligned, with 0xA5 canaries between them, and after each call
the whole pool image is compared with the expected one: stream rows untouched, every repair row exactly
blk_len[w] bytes, canaries intact.  Every address handed to a kernel comes from a live allocation (or is 0
where the interface says the row is never dereferenced).

The shapes are the smallest at which the 2 KiB chunks of the shared-coefficient kernel can go wrong: width
48 (42 windows per chunk, a lane's two pieces in different windows), 1200, 2064 (a window over two chunks),
window counts that leave a partial last chunk, a single window."""
import numpy as np
import pytest

import test_xor_rows_gpu as XR
from oracle_py import Oracle

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEV = "cuda:0"
to_dev = XR.to_dev


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


def starts(kind, k, nwin):
    """Window start rows: 'overlap' step 1, 'adjacent' step k, 'mixed' several runs out of order with a gap
    and a repeated window."""
    if kind == "overlap":
        return list(range(nwin))
    if kind == "adjacent":
        return [w * k for w in range(nwin)]
    n = max(nwin // 4, 1)
    a = list(range(0, n))                                    # step 1
    b = [n + k + 3 + 2 * w for w in range(n)]                # after a gap, step 2
    c = [b[-1] + k + w * k for w in range(n)]                # adjacent
    out = c + a + b                                          # the runs out of order
    out += [a[len(a) // 2]] * 2                              # a repeated window
    while len(out) < nwin:
        out.append(out[len(out) % 7])
    return out[:nwin]


class Case:
    """A stream of ragged rows and nwin windows over it.  equal: every length is S (the packed baseline)."""

    def __init__(self, oracle, S, k, r, kind, nwin, seed, equal=False):
        rng = np.random.default_rng(seed)
        self.S, self.k, self.r, self.nwin = S, k, r, nwin
        self.wrow = np.array(starts(kind, k, nwin), np.uint32)
        self.nrows = nrows = int(self.wrow.max()) + k
        cand = sorted({min(max(x, 0), S) for x in (0, 1, 3, 4, 15, 16, 17, S - 1, S)})
        if equal:
            lens = [S] * nrows
        else:
            lens = [cand[x % len(cand)] if rng.random() < 0.4 else int(rng.integers(0, S + 1)) for x in range(nrows)]
            if nrows >= 3:
                lens[nrows - 1] = 0      # a row of 0 bytes: its address is 0
            lens[int(self.wrow[0])] = S  # window 0 holds a full row
        bcand = sorted({min(max(x, 1), S) for x in (1, 3, 4, 15, 16, 17, S - 1, S)})
        blk = []
        for w in range(nwin):
            ws = int(self.wrow[w])
            mx = max(lens[ws:ws + k])
            if equal:
                blk.append(S)
            elif w % 3 == 0:
                blk.append(mx)                          # the reference's max_length (0: nothing is written)
            else:
                blk.append(bcand[(w // 3) % len(bcand)])  # any length: longer rows are truncated for this window
        if not equal and nwin > 1:
            blk[1] = max(1, S // 2 - 1)                 # window 1: shorter than a row it holds
            lens[int(self.wrow[1])] = S
        self.longer = [(w, x) for w in range(nwin) for x in range(int(self.wrow[w]), int(self.wrow[w]) + k)
                       if lens[x] > blk[w]]
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
            bl, ws = blk[w], int(self.wrow[w])
            if not bl:
                continue
            srcs = [self.rows[x][:bl] for x in range(ws, ws + k)]
            if max(len(s) for s in srcs) < bl:  # zero-padding to the window's length changes no repair byte
                srcs[0] = np.concatenate([srcs[0], np.zeros(bl - len(srcs[0]), np.uint8)])
            ret, reps = oracle.rlc_encode_block(0, srcs, r)
            assert ret == 0 and all(len(x) == bl for x in reps)
            for i in range(r):
                o = self.rep_off[w * r + i]
                self.want[o:o + bl] = reps[i]

    def tables(self, base):
        return {"rows": XR._addr(base, self.row_off), "row_len": self.row_len, "wrow": self.wrow,
                "rep_rows": XR._addr(base, self.rep_off), "blk_len": self.blk_len}


# S, k, r, window starts, nwin
SHAPES = [
    (48, 4, 2, "overlap", 300),     # 14400 B of windows: 7 chunks and a partial one
    (48, 1, 1, "adjacent", 131),
    (48, 30, 3, "mixed", 203),
    (44, 4, 5, "mixed", 100),       # symbol_size below the width of 48
    (48, 4, 8, "overlap", 1),       # a single window, less than one chunk
    (1200, 4, 5, "overlap", 67),
    (1200, 30, 8, "mixed", 41),
    (1200, 4, 9, "adjacent", 33),   # a tile of 8 and a remainder
    (1200, 1, 2, "mixed", 19),
    (2064, 4, 1, "overlap", 5),     # a window spans chunks
    (2064, 30, 9, "mixed", 9),
    (2064, 1, 3, "adjacent", 1),
]

_cases = {}


def case(oracle, *shape, equal=False):
    """One reference per shape, shared by the tests and never modified."""
    key = shape + (equal,)
    if key not in _cases:
        S, k, r, kind, nwin = shape
        _cases[key] = Case(oracle, S, k, r, kind, nwin, 31 * S + 7 * k + r + nwin, equal)
    return _cases[key]


def run_device(eng, c, clamp=False):
    pool = to_dev(c.image)
    t = c.tables(pool.data_ptr())
    if clamp:  # the kernels clamp: a window length above symbol_size, a row length above it
        t["blk_len"], t["row_len"] = t["blk_len"].copy(), t["row_len"].copy()
        full = np.flatnonzero(c.blk_len == c.S)
        if len(full):
            t["blk_len"][full[0]] = c.S + 100
        if c.S % 16 == 0:
            t["row_len"][np.flatnonzero(c.row_len == c.S)[0]] = c.S + 52
    eng.rlc_window_encode_rows(to_dev(t["rows"]), to_dev(t["row_len"]), c.nrows, to_dev(t["wrow"]),
                               to_dev(t["rep_rows"]), to_dev(t["blk_len"]), c.nwin, c.k, c.r, c.S)
    torch.cuda.synchronize()
    return pool.cpu().numpy()


@pytest.mark.parametrize("S,k,r,kind,nwin", SHAPES)
def test_device_form_matches_the_oracle(eng, oracle, S, k, r, kind, nwin):
    c = case(oracle, S, k, r, kind, nwin)
    if nwin > 1:
        assert c.longer, "the case holds a row longer than one of its windows"
    if c.nrows >= 3:
        assert any(o is None for o in c.row_off), "the case holds a row of 0 bytes at address 0"
    got = run_device(eng, c, clamp=True)
    bad = np.flatnonzero(got != c.want)
    assert not len(bad), (S, k, r, kind, nwin, bad[:8])


def test_a_window_of_length_0_writes_nothing(eng, oracle):
    c = Case(oracle, 48, 4, 2, "overlap", 50, 5)
    c.blk_len = c.blk_len.copy()
    for w in (0, 7, 49):  # their repair rows keep their canaries; the addresses given are never dereferenced
        for i in range(c.r):
            o = c.rep_off[w * c.r + i]
            if o is not None:
                c.want[o:o + int(c.blk_len[w])] = XR.GUARD
                c.rep_off[w * c.r + i] = None
        c.blk_len[w] = 0
    got = run_device(eng, c)
    assert np.array_equal(got, c.want), np.flatnonzero(got != c.want)[:8]


@pytest.mark.parametrize("S,k,r,kind,nwin", [s for s in SHAPES if s[0] % 16 == 0 and s[4] > 1][::2])
def test_equal_lengths_match_the_packed_table_kernel(eng, oracle, S, k, r, kind, nwin):
    c = case(oracle, S, k, r, kind, nwin, equal=True)
    got = run_device(eng, c)
    assert np.array_equal(got, c.want)
    packed = to_dev(np.stack(c.rows))
    rep = torch.full((nwin, r, S), XR.GUARD, dtype=torch.uint8, device=DEV)
    eng.rlc_window_encode_table(packed, c.nrows, to_dev(c.wrow), rep, nwin, k, r, S)
    torch.cuda.synchronize()
    rep = rep.cpu().numpy().reshape(nwin * r, S)
    for x, o in enumerate(c.rep_off):
        assert np.array_equal(got[o:o + S], rep[x]), x


def test_refusals_on_the_device(eng, oracle):
    from pquic_amd.engine import FecGpuError
    c = case(oracle, 48, 4, 2, "overlap", 300)
    with eng.knob("window_sc", 0):
        with pytest.raises(FecGpuError, match="window_sc"):
            run_device(eng, c)
    with pytest.raises(FecGpuError, match="workspace"):
        pool = to_dev(c.image)
        t = {n: to_dev(v) for n, v in c.tables(pool.data_ptr()).items()}
        eng.rlc_window_encode_rows(t["rows"], t["row_len"], c.nrows, t["wrow"], t["rep_rows"], t["blk_len"], c.nwin,
                                   c.k, c.r, c.S, workspace=torch.empty(c.nrows * 48 - 16, dtype=torch.uint8, device=DEV))


# ---------------------------------------------------------------------------------- the host form
HOST_SHAPES = [(48, 30, 3, "mixed", 203), (1200, 4, 9, "adjacent", 33), (2064, 4, 1, "overlap", 5)]


def run_host(eng, hostpath, c, pinned=True, pageable=(), registered=False):
    """The host form on fresh buffers: rows in fecgpu_host_alloc memory or in a registered range of ordinary
    memory, the tables page-locked or pageable numpy arrays."""
    lib = eng.lib
    hm = XR.HostMem(lib, True)
    raw = None
    try:
        if registered:
            page = 4096
            size = (len(c.image) + page - 1) // page * page
            raw = np.zeros(size + page, np.uint8)
            off = (-raw.ctypes.data) % page
            pool = raw[off:off + len(c.image)]
            pool[:] = c.image
            assert lib.fecgpu_host_register(pool.ctypes.data, size) == 0
        else:
            pool = hm.array(c.image)
        t = {n: hm.array(v, pinned=pinned and n not in pageable) for n, v in c.tables(XR._dev_addr(lib, pool)).items()}
        hostpath.rlc_window_encode_rows(t["rows"], t["row_len"], c.nrows, t["wrow"], t["rep_rows"], t["blk_len"],
                                        c.nwin, c.k, c.r, c.S)
        return pool.copy()
    finally:
        if raw is not None:
            assert lib.fecgpu_host_unregister(pool.ctypes.data) == 0
        hm.close()


@pytest.mark.parametrize("S,k,r,kind,nwin", HOST_SHAPES)
@pytest.mark.parametrize("mode", ["pinned", "one_pageable", "pageable", "registered", "fallback"])
def test_host_form_matches_the_oracle(eng, oracle, hostpath, mode, S, k, r, kind, nwin):
    c = case(oracle, S, k, r, kind, nwin)
    if mode == "fallback":  # knob window_sc 0: the windows as blocks through the one-pass row kernels
        with eng.knob("window_sc", 0):
            got = run_host(eng, hostpath, c)
    else:
        got = run_host(eng, hostpath, c, pinned=mode != "pageable", pageable=("blk_len",) if mode == "one_pageable" else (),
                       registered=mode == "registered")
    bad = np.flatnonzero(got != c.want)
    assert not len(bad), (mode, bad[:8])


def test_host_form_refuses_bad_tables_with_a_context(eng, oracle, hostpath):
    c = case(oracle, 48, 4, 2, "overlap", 300)
    t = c.tables(0)
    lib = eng.lib

    def call(**kw):
        a = {n: np.ascontiguousarray(kw.get(n, v)) for n, v in t.items()}
        return lib.fecgpu_rlc_window_encode_rows_host(hostpath.ctx, a["rows"].ctypes.data, a["row_len"].ctypes.data,
                                                      c.nrows, a["wrow"].ctypes.data, a["rep_rows"].ctypes.data,
                                                      a["blk_len"].ctypes.data, c.nwin, c.k, c.r, c.S)
    bad = c.wrow.copy()
    bad[5] = c.nrows - c.k + 1
    assert call(wrow=bad) == -1 and "wrow" in eng.err()
    bad = c.row_len.copy()
    bad[3] = c.S + 1
    assert call(row_len=bad) == -1 and "row_len" in eng.err()
    bad = c.blk_len.copy()
    bad[-1] = c.S + 4
    assert call(blk_len=bad) == -1 and "blk_len" in eng.err()
