"""The six host forms that take row tables (fecgpu_rlc_encode_rows_host, fecgpu_rlc_decode_rows_host,
fecgpu_rlc_encode_rows_len_host, fecgpu_rlc_decode_rows_len_host, fecgpu_xor_encode_rows_host,
fecgpu_xor_decode_rows_host) where they differ from one another: a call cut into slices gives the bytes of
the call launched whole, one pageable array among page-locked ones sends every array through the staged
copies, and a decode without repairs takes NULL repair tables.  The reference is always the device entry
point of the same form on the whole batch (and the CPU oracle where the batch builders of
test_rows_len_gpu.py and test_xor_rows_gpu.py carry its verdict).  Byte work: every comparison is exact,
over the whole pool the rows live in."""
import ctypes as C

import numpy as np
import pytest

import test_rows_len_gpu as RL
import test_xor_rows_gpu as XR
from oracle_py import Oracle

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEV = "cuda:0"
CANARY = 0xC3
SEED = 20261020
FORMS = ("rlc_encode_rows", "rlc_decode_rows", "rlc_encode_rows_len", "rlc_decode_rows_len", "xor_encode_rows",
         "xor_decode_rows")


@pytest.fixture(scope="module")
def eng():
    from pquic_amd import Engine
    if not torch.cuda.is_available():
        pytest.fail("GPU test run without a visible GPU")
    e = Engine(0)
    e.lib.fecgpu_rlc_encode_rows_host.argtypes = [C.c_void_p] * 3 + [C.c_uint64] + [C.c_uint32] * 3 + [C.c_void_p]
    return e


@pytest.fixture(scope="module")
def oracle():
    return Oracle()


@pytest.fixture(scope="module")
def hostpath(eng):
    from pquic_amd.engine import HostPath
    hp = HostPath(0, nstreams=2, chunk_bytes=1 << 20)
    yield hp
    hp.close()


def _p(x):
    if x is None:
        return None
    return x.data_ptr() if hasattr(x, "data_ptr") else x.ctypes.data


def _rows(base, first, n, L):
    return (base + first + np.arange(n, dtype=np.int64) * L).astype(np.uint64)


# ---------------------------------------------------------------------------------- the six forms
# A form is one batch for one entry point: `image`, the pool its rows live in; arrays(base), its per-block
# arrays by name (None: not given) for a pool at device address `base`; `order`, the names in the order
# the host entry point looks them up; host() and device(), the two calls; `want`, the oracle's verdict on
# the pool where the batch builder has one.
class EncodeRows:
    order = ("src_rows", "rep_rows", "fbn")
    want = None

    def __init__(self, rng, eng, oracle, nb, k, r, L, fbn=True):
        self.d = (nb, k, r, L)
        self.image = np.full(nb * (k + r) * L + 64, CANARY, np.uint8)
        self.image[:nb * k * L] = rng.integers(0, 256, nb * k * L, dtype=np.uint8)
        self.fbn = rng.integers(0, 1 << 24, nb).astype(np.uint32) if fbn else None

    def arrays(self, base):
        nb, k, r, L = self.d
        return {"src_rows": _rows(base, 0, nb * k, L), "rep_rows": _rows(base, nb * k * L, nb * r, L), "fbn": self.fbn}

    def host(self, lib, ctx, a):
        return lib.fecgpu_rlc_encode_rows_host(ctx, _p(a["src_rows"]), _p(a["rep_rows"]), *self.d, _p(a["fbn"]))

    def device(self, eng, a):
        eng.rlc_encode_rows(a["src_rows"], a["rep_rows"], *self.d, fbn_base=0, fbn=a["fbn"])


class DecodeRows:
    """Equal-length rows, repairs seeded (fbn << 8) | i.  Blocks by turns: complete, then 1 .. min(k, r)
    sources missing (one, with r == 0), their rows holding garbage; one block lacks a repair."""
    order = ("src_rows", "rep_rows", "seeds", "sp", "rp", "status", "recovered")
    want = None

    def __init__(self, rng, eng, oracle, nb, k, r, L):
        self.d = (nb, k, r, L)
        src = rng.integers(0, 256, (nb, k, L), dtype=np.uint8)
        fbn = rng.integers(0, 1 << 24, nb).astype(np.uint32)
        rep = torch.empty((nb, r, L), dtype=torch.uint8, device=DEV)
        if r:
            eng.rlc_encode(RL.to_dev(src), rep, k, r, L, fbn=RL.to_dev(fbn))
            torch.cuda.synchronize()
        self.seeds = ((fbn.astype(np.uint64)[:, None] << 8) | np.arange(r, dtype=np.uint64)[None, :]).astype(np.uint32)
        self.sp, self.rp = np.zeros((nb, 2), np.uint64), np.zeros((nb, 2), np.uint64)
        for b in range(nb):
            present = np.ones(k, bool)
            if b % 4:
                present[rng.choice(k, 1 + b % max(min(k, r), 1), replace=False)] = False
            src[b, ~present] = 0xA5
            self.sp[b] = RL.mask(present, k)
            self.rp[b] = RL.mask([not (b == 5 and i == 0) for i in range(r)], r)
        self.image = np.concatenate([src.reshape(-1), rep.cpu().numpy().reshape(-1), np.full(64, CANARY, np.uint8)])

    def arrays(self, base):
        nb, k, r, L = self.d
        return {"src_rows": _rows(base, 0, nb * k, L), "rep_rows": _rows(base, nb * k * L, nb * r, L) if r else None,
                "seeds": self.seeds.reshape(-1) if r else None, "sp": self.sp.reshape(-1), "rp": self.rp.reshape(-1),
                "status": np.full(nb, 0xEE, np.uint8), "recovered": np.full(2 * nb, 2 ** 64 - 1, np.uint64)}

    def host(self, lib, ctx, a):
        return lib.fecgpu_rlc_decode_rows_host(ctx, _p(a["src_rows"]), _p(a["rep_rows"]), *self.d, _p(a["seeds"]),
                                               _p(a["sp"]), _p(a["rp"]), _p(a["status"]), _p(a["recovered"]))

    def device(self, eng, a):
        nb, k, r, L = self.d
        ws = eng.alloc_workspace(nb, k, r)
        # the device form refuses a NULL repair table even when it has no entries: the source table stands in
        rc = eng.lib.fecgpu_rlc_decode_rows(_p(a["src_rows"]), _p(a["rep_rows"] if r else a["src_rows"]), nb, k, r, L,
                                            _p(a["seeds"]), _p(a["sp"]), _p(a["rp"]), _p(a["status"]),
                                            _p(a["recovered"]), _p(ws), ws.numel(), eng._stream(None))
        assert rc == 0, eng.err()


class EncodeRowsLen:
    order = ("src_rows", "rep_rows", "src_len", "blk_len", "fbn")

    def __init__(self, rng, eng, oracle, nb, k, r, L, fbn=True):
        self.d = (nb, k, r, L)
        self.g, self.fbn, self.image, self.want = RL._encode_case(rng, oracle, nb, k, r, L)
        if not fbn:  # the oracle's repairs were made for fbn[]
            self.fbn = self.want = None

    def arrays(self, base):
        rows_s, src_len, rows_r, blk = RL._encode_tables(self.g, base)
        return {"src_rows": rows_s, "src_len": src_len, "rep_rows": rows_r, "blk_len": blk, "fbn": self.fbn}

    def host(self, lib, ctx, a):
        return lib.fecgpu_rlc_encode_rows_len_host(ctx, _p(a["src_rows"]), _p(a["src_len"]), _p(a["rep_rows"]),
                                                   _p(a["blk_len"]), *self.d, _p(a["fbn"]))

    def device(self, eng, a):
        eng.rlc_encode_rows_len(a["src_rows"], a["src_len"], a["rep_rows"], a["blk_len"], *self.d, fbn_base=0,
                                fbn=a["fbn"])


class DecodeRowsLen:
    order = ("src_rows", "src_len", "blk_len", "rep_rows", "rep_len", "seeds", "sp", "rp", "status", "recovered")
    want = None

    def __init__(self, rng, eng, oracle, nb, k, r, L):
        self.d = (nb, k, r, L)
        if r:
            self.c = c = RL.make_decode_case(rng, oracle, nb, k, r, L)
            self.image, self.want = c.pool_h, c.want
            self.t = c.tables
            return
        # no repairs: ragged sources, every other block with one of them missing
        g = RL.Ragged(rng, nb, k, 0, L, decode=True)
        present = np.ones((nb, k), bool)
        present[np.arange(1, nb, 2), rng.integers(0, k, nb // 2)] = False
        self.image = g.pool.bytes()
        g.fill_sources(self.image, present)
        sp = np.stack([RL.mask(present[b], k) for b in range(nb)]).reshape(-1)
        self.t = lambda base: ((base + g.src_off.reshape(-1)).astype(np.uint64), g.src_len.reshape(-1).copy(), None,
                               None, g.blk.copy(), None, sp, np.zeros(2 * nb, np.uint64))

    def arrays(self, base):
        nb = self.d[0]
        t = self.t(base)
        return {"src_rows": t[0], "src_len": t[1], "rep_rows": t[2], "rep_len": t[3], "blk_len": t[4], "seeds": t[5],
                "sp": t[6], "rp": t[7], "status": np.full(nb, 0xEE, np.uint8),
                "recovered": np.full(2 * nb, 2 ** 64 - 1, np.uint64)}

    def host(self, lib, ctx, a):
        return lib.fecgpu_rlc_decode_rows_len_host(ctx, _p(a["src_rows"]), _p(a["src_len"]), _p(a["rep_rows"]),
                                                   _p(a["rep_len"]), _p(a["blk_len"]), *self.d, _p(a["seeds"]),
                                                   _p(a["sp"]), _p(a["rp"]), _p(a["status"]), _p(a["recovered"]))

    def device(self, eng, a):
        # as in DecodeRows.device: with r == 0 the source table stands in for the repair table
        eng.rlc_decode_rows_len(a["src_rows"], a["src_len"], a["rep_rows"] if self.d[2] else a["src_rows"],
                                a["rep_len"], a["blk_len"], a["seeds"], a["sp"], a["rp"], a["status"], a["recovered"],
                                *self.d)


class XorEncodeRows:
    order = ("src_rows", "rep_rows", "src_len", "blk_len")

    def __init__(self, rng, eng, oracle, nb, k, r, L):
        self.c = c = XR.EncodeCase(oracle, k, L, nb - 2, int(rng.integers(1 << 30)))  # two special blocks follow
        assert c.nb == nb
        self.d, self.image, self.want = (nb, k, L), c.image, c.want

    def arrays(self, base):
        rows, reps = self.c.tables(base)
        return {"src_rows": rows, "src_len": self.c.src_len, "rep_rows": reps, "blk_len": self.c.blk_len}

    def host(self, lib, ctx, a):
        return lib.fecgpu_xor_encode_rows_host(ctx, _p(a["src_rows"]), _p(a["src_len"]), _p(a["rep_rows"]),
                                               _p(a["blk_len"]), *self.d)

    def device(self, eng, a):
        eng.xor_encode_rows(a["src_rows"], a["src_len"], a["rep_rows"], a["blk_len"], *self.d)


class XorDecodeRows:
    order = ("src_rows", "src_len", "blk_len", "rep_rows", "sp", "rp", "status", "recovered")

    def __init__(self, rng, eng, oracle, nb, k, r, L):
        self.c = c = XR.DecodeCase(oracle, k, L, nb, int(rng.integers(1 << 30)), longer=False)
        self.d, self.image, self.want = (nb, k, L), c.image, c.want

    def arrays(self, base):
        nb = self.d[0]
        rows, reps = self.c.tables(base)
        return {"src_rows": rows, "src_len": self.c.src_len, "rep_rows": reps, "blk_len": self.c.blk_len,
                "sp": self.c.sp.reshape(-1), "rp": self.c.rp.reshape(-1), "status": np.full(nb, 0xEE, np.uint8),
                "recovered": np.full(2 * nb, 2 ** 64 - 1, np.uint64)}

    def host(self, lib, ctx, a):
        return lib.fecgpu_xor_decode_rows_host(ctx, _p(a["src_rows"]), _p(a["src_len"]), _p(a["rep_rows"]),
                                               _p(a["blk_len"]), *self.d, _p(a["sp"]), _p(a["rp"]), _p(a["status"]),
                                               _p(a["recovered"]))

    def device(self, eng, a):
        eng.xor_decode_rows(a["src_rows"], a["src_len"], a["rep_rows"], a["blk_len"], a["sp"], a["rp"], a["status"],
                            a["recovered"], *self.d)


CLASSES = dict(zip(FORMS, (EncodeRows, DecodeRows, EncodeRowsLen, DecodeRowsLen, XorEncodeRows, XorDecodeRows)))


def make_form(name, eng, oracle, nb, k, r, L, **kw):
    rng = np.random.default_rng([SEED, FORMS.index(name), nb, k, r, L])
    form = CLASSES[name](rng, eng, oracle, nb, k, r, L, **kw)
    assert set(form.order) == set(form.arrays(0))
    return form


# ---------------------------------------------------------------------------------- the two runs
class Out:
    """What a call left: the pool, status and recovered (None for an encode), and what it counted."""

    def __init__(self, pool, a, s0=None, s1=None):
        self.pool = pool
        self.status, self.recovered = a.get("status"), a.get("recovered")
        if s0:
            self.slices = s1["yield_slices"] - s0["yield_slices"]
            self.hits = s1["pinned_registry_hits"] - s0["pinned_registry_hits"]
            self.misses = s1["pinned_registry_misses"] - s0["pinned_registry_misses"]


def assert_same(got, ref, tag):
    assert np.array_equal(got.pool, ref.pool), (tag, np.flatnonzero(got.pool != ref.pool)[:8])
    if ref.status is not None:
        assert np.array_equal(got.status, ref.status), (tag, np.flatnonzero(got.status != ref.status)[:8])
        assert np.array_equal(got.recovered, ref.recovered), (tag, np.flatnonzero(got.recovered != ref.recovered)[:8])


def run_host(eng, hostpath, form, tables_pinned, pageable=()):
    """The host form on fresh buffers: the rows page-locked, the per-block arrays page-locked or pageable
    numpy arrays (`pageable`: the names that are pageable among page-locked ones)."""
    lib = eng.lib
    hm = XR.HostMem(lib, True)
    try:
        pool = hm.array(form.image)
        a = {n: None if v is None else hm.array(v, pinned=tables_pinned and n not in pageable)
             for n, v in form.arrays(XR._dev_addr(lib, pool)).items()}
        s0 = eng.stats()
        rc = form.host(lib, hostpath.ctx, a)
        s1 = eng.stats()
        assert rc == 0, (rc, eng.err())
        return Out(pool.copy(), {n: v.copy() for n, v in a.items() if v is not None}, s0, s1)
    finally:
        hm.close()


def run_device(eng, form):
    """The device entry point of the same form, the whole batch in one call, everything in device memory."""
    pool = RL.to_dev(form.image)
    a = {n: None if v is None else RL.to_dev(v) for n, v in form.arrays(pool.data_ptr()).items()}
    form.device(eng, a)
    torch.cuda.synchronize()
    out = Out(pool.cpu().numpy(), {n: v.cpu().numpy() for n, v in a.items() if v is not None})
    if out.recovered is not None:
        out.recovered = out.recovered.view(np.uint64)
    if form.want is not None:
        assert np.array_equal(out.pool, form.want), "the device form differs from the oracle"
    return out


# ---------------------------------------------------------------------------------- the tests
@pytest.mark.parametrize("name,fbn", [(n, True) for n in FORMS] + [("rlc_encode_rows", False), ("rlc_encode_rows_len", False)])
def test_sliced_equals_unsliced(eng, oracle, hostpath, name, fbn):
    """100 blocks of k4 r2 L1200 (ragged for the four newer forms), everything page-locked.  With yield_always
    and a 1 KiB slice the Pacer cuts at its floor of 32 blocks: slices of 32, 32, 32 and 4 over two streams.
    The same call with yield_slice_kb 0 is not cut.  Both leave the bytes, status and masks of the device
    form on the whole batch; without fbn[] that pins that the slice at b0 codes block numbers b0 ..."""
    nb, k, r, L = 100, 4, 2, 1200
    kw = {} if fbn else {"fbn": False}
    form = make_form(name, eng, oracle, nb, k, r, L, **kw)
    if not fbn:
        assert form.arrays(0)["fbn"] is None
    old = {n: eng.get_knob(n) for n in ("yield_always", "yield_slice_kb")}
    try:
        eng.set_knob("yield_always", 1)
        eng.set_knob("yield_slice_kb", 1)
        cut = run_host(eng, hostpath, form, True)
        eng.set_knob("yield_slice_kb", 0)
        whole = run_host(eng, hostpath, form, True)
    finally:
        for n, v in old.items():
            eng.set_knob(n, v)
    assert cut.slices >= 4 and whole.slices == 0, (cut.slices, whole.slices)
    assert_same(cut, whole, "sliced against unsliced")
    assert_same(cut, run_device(eng, form), "sliced against the device form")
    if cut.status is not None:
        assert 0xEE not in cut.status


@pytest.mark.parametrize("name", FORMS)
def test_one_pageable_array_stages_them_all(eng, oracle, hostpath, name):
    """65 blocks of k16 r4 L1200 (two sub-batches at 1 MiB), rows page-locked.  Every per-block array is
    page-locked but the one the entry point looks up last, a pageable numpy array: the call must take the
    staged copies for all of them (all or nothing) and give what the all-pageable call gives -- status and
    recovered in the caller's arrays.  The registry saw every array before the last (hits) and missed once."""
    form = make_form(name, eng, oracle, 65, 16, 4, 1200)
    last = form.order[-1]
    pageable = run_host(eng, hostpath, form, False)
    mixed = run_host(eng, hostpath, form, True, pageable=(last,))
    assert_same(mixed, pageable, f"{last} pageable against all pageable")
    assert_same(mixed, run_device(eng, form), f"{last} pageable against the device form")
    assert (mixed.hits, mixed.misses) == (len(form.order) - 1, 1), (mixed.hits, mixed.misses)
    assert mixed.slices == 0 and pageable.slices == 0
    if mixed.status is not None:
        assert 0xEE not in mixed.status


@pytest.mark.parametrize("tables_pinned", [False, True])
@pytest.mark.parametrize("name", ["rlc_decode_rows", "rlc_decode_rows_len"])
def test_decode_without_repairs(eng, oracle, hostpath, name, tables_pinned):
    """r == 0 with NULL rep_rows, rep_len and seeds, 33 blocks of k4 L36, some with a missing source: status,
    recovered masks and rows as the device form gives them, tables pageable and page-locked."""
    nb, k = 33, 4
    form = make_form(name, eng, oracle, nb, k, 0, 36)
    a = form.arrays(0)
    assert a["rep_rows"] is None and a["seeds"] is None and a.get("rep_len") is None
    complete = (a["sp"].reshape(nb, 2)[:, 0] & np.uint64((1 << k) - 1)) == np.uint64((1 << k) - 1)
    assert 0 < complete.sum() < nb
    got = run_host(eng, hostpath, form, tables_pinned)
    assert_same(got, run_device(eng, form), f"r == 0, tables page-locked: {tables_pinned}")
    assert 0xEE not in got.status
    assert np.array_equal(got.pool, form.image), "a decode without repairs wrote a row"
