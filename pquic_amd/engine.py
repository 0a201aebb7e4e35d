"""ctypes mirror of include/fecgpu.h (batched device-resident FEC engine).

Buffers are torch CUDA tensors (HBM allocations) or raw device addresses; kernels run on
the given HIP stream (default: torch's current stream), so torch.cuda.Event timing
brackets exactly the engine's launches.
"""
from __future__ import annotations

import ctypes as C
import os

PKG = os.path.dirname(os.path.abspath(__file__))
# PQUIC_AMD_LIB selects another in-tree build of the same library (A/B experiments, tools/)
LIB_PATH = os.environ.get("PQUIC_AMD_LIB") or os.path.join(PKG, "lib", "libpquic_fec.so")

OK, ERR_INVALID, ERR_HIP, ERR_NO_DEVICE, ERR_NOMEM = 0, -1, -2, -3, -4
BLOCK_RECOVERED, BLOCK_NOTHING, BLOCK_REF_UB, BLOCK_SINGULAR = 0, 1, 2, 3

_lib = None


class FecGpuError(RuntimeError):
    pass


class FecGpuStats(C.Structure):
    _fields_ = [("encode_calls", C.c_uint64), ("encode_blocks", C.c_uint64),
                ("decode_calls", C.c_uint64), ("decode_blocks", C.c_uint64),
                ("pinned_registry_hits", C.c_uint64), ("pinned_registry_misses", C.c_uint64),
                ("yield_slices", C.c_uint64), ("yield_waits", C.c_uint64)]


def load_library(path: str = LIB_PATH, private: bool = False):
    """Load libpquic_fec.so.  Raises if it is missing -- never falls back to CPU.
    private=True loads another build side by side (its own handle; in-process A/B tools)."""
    global _lib
    if _lib is not None and not private:
        return _lib
    if not os.path.exists(path):
        raise FecGpuError(f"{path} not built: run `python -c 'import __graft_entry__ as g; g.build()'`")
    L = C.CDLL(path)
    v, u64, u32, sz = C.c_void_p, C.c_uint64, C.c_uint32, C.c_size_t
    L.fecgpu_init.argtypes = [C.c_int]
    L.fecgpu_version.restype = C.c_char_p
    L.fecgpu_last_error.restype = C.c_char_p
    L.fecgpu_rlc_encode.argtypes = [v, v, u64, u32, u32, u32, u32, v, v]
    L.fecgpu_xor_encode.argtypes = [v, v, u64, u32, u32, v]
    L.fecgpu_rlc_window_encode.argtypes = [v, u64, u32, u32, u32, u32, v, v]
    L.fecgpu_write_repair_frames.argtypes = [v, u64, u32, u32, C.c_uint16, u32, v, C.c_uint8, C.c_uint8, v, u32, v]
    L.fecgpu_rlc_decode_workspace.argtypes = [u64, u32, u32]
    L.fecgpu_rlc_decode_workspace.restype = sz
    L.fecgpu_rlc_decode.argtypes = [v, v, u64, u32, u32, u32, u32, v, v, v, v, v, v, sz, v]
    L.fecgpu_xor_decode.argtypes = [v, v, u64, u32, u32, v, v, v, v, v]
    if hasattr(L, "fecgpu_xor_decode_to") or not private:  # a private (A/B) load may be an older build
        L.fecgpu_xor_decode_to.argtypes = [v, v, v, u64, u32, u32, v, v, v, v, v]
    L.fecgpu_rlc_decode_plan.argtypes = [u64, u32, u32, u32, v, v, v, v, sz, v]
    L.fecgpu_rlc_decode_plan_seeded.argtypes = [u64, u32, u32, v, v, v, v, sz, v]
    L.fecgpu_rlc_decode_seeded.argtypes = [v, v, u64, u32, u32, u32, v, v, v, v, v, v, sz, v]
    L.fecgpu_rlc_decode_apply.argtypes = [v, v, u64, u32, u32, u32, v, v, v, sz, v]
    L.fecgpu_rlc_decode_apply_to.argtypes = [v, v, v, u64, u32, u32, u32, v, v, v, sz, v]
    if private and not hasattr(L, "fecgpu_rlc_decode_apply_packed"):  # an older build (A/B baselines)
        pass
    else:
        L.fecgpu_rlc_decode_apply_packed.argtypes = [v, v, v, u64, u32, u32, u32, v, v, v, sz, v]
    L.fecgpu_synth_fill.argtypes = [v, u64, u64, u64, v]
    L.fecgpu_get_stats.argtypes = [C.POINTER(FecGpuStats)]
    L.fecgpu_set_knob.argtypes = [C.c_char_p, C.c_int]
    L.fecgpu_get_knob.argtypes = [C.c_char_p, C.POINTER(C.c_int)]
    L.fecgpu_host_ctx_create.argtypes = [C.c_int, C.c_int, sz]
    L.fecgpu_host_ctx_create.restype = v
    L.fecgpu_host_ctx_destroy.argtypes = [v]
    L.fecgpu_rlc_encode_host.argtypes = [v, v, v, u64, u32, u32, u32, u32, v]
    L.fecgpu_rlc_decode_host.argtypes = [v, v, v, u64, u32, u32, u32, u32, v, v, v, v, v]
    L.fecgpu_rlc_decode_host_seeded.argtypes = [v, v, v, u64, u32, u32, u32, v, v, v, v, v]
    L.fecgpu_xor_encode_host.argtypes = [v, v, v, u64, u32, u32]
    L.fecgpu_xor_decode_host.argtypes = [v, v, v, u64, u32, u32, v, v, v, v]
    if hasattr(L, "fecgpu_rlc_window_encode_host"):  # an older build (A/B baselines) may lack it
        L.fecgpu_rlc_window_encode_host.argtypes = [v, v, u64, v, u64, u32, u32, u32, v]
    L.fecgpu_host_register.argtypes = [v, sz]
    L.fecgpu_host_unregister.argtypes = [v]
    L.fecgpu_host_device_address.argtypes = [v, sz, C.POINTER(u64)]
    L.fecgpu_block_svc_create.argtypes = [C.c_int]
    L.fecgpu_block_svc_create.restype = v
    L.fecgpu_block_svc_destroy.argtypes = [v]
    L.fecgpu_block_svc_rlc_encode.argtypes = [v, v, v, u32, u32, u32, u32]
    L.fecgpu_block_svc_rlc_decode_seeded.argtypes = [v, v, v, v, u32, u32, u32, v, v, v, v, v]
    L.fecgpu_block_svc_launches.argtypes = [v]
    L.fecgpu_block_svc_launches.restype = u64
    if hasattr(L, "fecgpu_block_svc_set_deadline"):  # older builds (A/B baselines) lack these
        L.fecgpu_block_svc_set_deadline.argtypes = [v, u64]
        L.fecgpu_block_svc_deadline_misses.argtypes = [v]
        L.fecgpu_block_svc_deadline_misses.restype = u64
    if hasattr(L, "fecgpu_block_svc_last_stamps"):
        L.fecgpu_block_svc_last_stamps.argtypes = [v, C.POINTER(u64)]
    if hasattr(L, "fecgpu_block_svc_worker_running"):
        L.fecgpu_block_svc_worker_running.argtypes = [v]
    if hasattr(L, "fecgpu_rlc_decode_rows"):
        L.fecgpu_rlc_decode_rows.argtypes = [v, v, u64, u32, u32, u32, v, v, v, v, v, v, sz, v]
        L.fecgpu_rlc_decode_rows_host.argtypes = [v, v, v, u64, u32, u32, u32, v, v, v, v, v]
    if hasattr(L, "fecgpu_rlc_decode_full") or not private:  # a private (A/B) load may be an older build
        L.fecgpu_rlc_decode_plan_full.argtypes = [u64, u32, u32, u32, v, v, v, v, v, sz, v]
        L.fecgpu_rlc_decode_full.argtypes = [v, v, u64, u32, u32, u32, u32, v, v, v, v, v, v, v, sz, v]
        L.fecgpu_rlc_decode_host_full.argtypes = [v, v, v, u64, u32, u32, u32, u32, v, v, v, v, v, v]
    if hasattr(L, "fecgpu_rlc_encode_rows_len"):  # an older build (PQUIC_AMD_LIB, A/B baselines) lacks these
        L.fecgpu_rows_gather.argtypes = [v, v, u64, u32, v, v]
        L.fecgpu_rows_scatter.argtypes = [v, v, v, u64, u32, v]
        L.fecgpu_rlc_rows_len_workspace.argtypes = [u64, u32, u32, u32]
        L.fecgpu_rlc_rows_len_workspace.restype = sz
        L.fecgpu_rlc_encode_rows.argtypes = [v, v, u64, u32, u32, u32, u32, v, v]
        L.fecgpu_rlc_encode_rows_len.argtypes = [v, v, v, v, u64, u32, u32, u32, u32, v, v, sz, v]
        L.fecgpu_rlc_decode_rows_len.argtypes = [v, v, v, v, v, u64, u32, u32, u32, v, v, v, v, v, v, sz, v]
        L.fecgpu_rlc_encode_rows_len_host.argtypes = [v, v, v, v, v, u64, u32, u32, u32, v]
        L.fecgpu_rlc_decode_rows_len_host.argtypes = [v, v, v, v, v, v, u64, u32, u32, u32, v, v, v, v, v]
    if hasattr(L, "fecgpu_rlc_encode_rows_fused"):  # an older build (PQUIC_AMD_LIB, A/B baselines) lacks these
        L.fecgpu_rlc_encode_rows_fused.argtypes = [v, v, v, v, u64, u32, u32, u32, u32, v, v]
        L.fecgpu_rlc_decode_rows_fused.argtypes = [v, v, v, v, v, u64, u32, u32, u32, v, v, v, v, v, v, sz, v]
        L.fecgpu_rlc_encode_rows_fused_host.argtypes = [v, v, v, v, v, u64, u32, u32, u32, v]
        L.fecgpu_rlc_decode_rows_fused_host.argtypes = [v, v, v, v, v, v, u64, u32, u32, u32, v, v, v, v, v]
    if hasattr(L, "fecgpu_rlc_decode_rows_full"):  # an older build (PQUIC_AMD_LIB, A/B baselines) lacks these
        L.fecgpu_rlc_decode_rows_full.argtypes = L.fecgpu_rlc_decode_rows.argtypes
        L.fecgpu_rlc_decode_rows_host_full.argtypes = L.fecgpu_rlc_decode_rows_host.argtypes
        L.fecgpu_rlc_decode_rows_fused_full.argtypes = L.fecgpu_rlc_decode_rows_fused.argtypes
        L.fecgpu_rlc_decode_rows_fused_host_full.argtypes = L.fecgpu_rlc_decode_rows_fused_host.argtypes
        L.fecgpu_block_svc_rlc_decode_full.argtypes = L.fecgpu_block_svc_rlc_decode_seeded.argtypes
    if hasattr(L, "fecgpu_xor_encode_rows"):  # an older build (PQUIC_AMD_LIB, A/B baselines) lacks these
        L.fecgpu_xor_encode_rows.argtypes = [v, v, v, v, u64, u32, u32, v]
        L.fecgpu_xor_decode_rows.argtypes = [v, v, v, v, u64, u32, u32, v, v, v, v, v]
        L.fecgpu_xor_encode_rows_host.argtypes = [v, v, v, v, v, u64, u32, u32]
        L.fecgpu_xor_decode_rows_host.argtypes = [v, v, v, v, v, u64, u32, u32, v, v, v, v]
    if hasattr(L, "fecgpu_rlc_window_encode_rows"):  # an older build (PQUIC_AMD_LIB, A/B baselines) lacks these
        L.fecgpu_rlc_window_rows_workspace.argtypes = [u64, u32]
        L.fecgpu_rlc_window_rows_workspace.restype = sz
        L.fecgpu_rlc_window_encode_rows.argtypes = [v, v, u64, v, v, v, u64, u32, u32, u32, v, sz, v]
        L.fecgpu_rlc_window_encode_rows_host.argtypes = [v, v, v, u64, v, v, v, u64, u32, u32, u32]
    if hasattr(L, "fecgpu_rlc_window_encode_rows_var_host"):  # an older build (PQUIC_AMD_LIB, A/B baselines) lacks these
        L.fecgpu_rlc_window_encode_rows_var_host.argtypes = [v, v, v, u64, v, v, v, v, u64, u32, u32, u32]
        L.fecgpu_rlc_window_classes.argtypes = [v, u64, u32, u32, v, v, C.POINTER(u32), C.POINTER(u64)]
    if hasattr(L, "fecgpu_block_svc_rlc_encode_rows"):  # an older build (PQUIC_AMD_LIB, A/B baselines) lacks these
        L.fecgpu_block_svc_rlc_encode_rows.argtypes = [v, v, v, v, u32, u32, u32, u32]
        L.fecgpu_block_svc_rlc_decode_rows.argtypes = [v, v, v, v, v, u32, u32, u32, v, v, v, C.c_int, v, v]
        L.fecgpu_block_svc_xor_encode_rows.argtypes = [v, v, v, u64, u32, u32]
        L.fecgpu_block_svc_xor_decode_rows.argtypes = [v, v, v, u64, u32, u32, v, v, v, v]
    if hasattr(L, "fecgpu_rlc_span_decode") or not private:  # a private (A/B) load may be an older build
        L.fecgpu_rlc_span_decode_plan.argtypes = [u64, u32, u32, v, v, v, v, v, v, sz, v]
        L.fecgpu_rlc_span_decode.argtypes = [v, v, u64, u32, u32, u32, v, v, v, v, v, v, v, v, sz, v]
        L.fecgpu_rlc_span_decode_rows_fused.argtypes = [v, v, v, v, v, u64, u32, u32, u32, v, v, v, v, v, v, v, v,
                                                        sz, v]
        L.fecgpu_rlc_span_decode_rows_fused_host.argtypes = [v, v, v, v, v, v, u64, u32, u32, u32, v, v, v, v, v, v,
                                                             v]
        L.fecgpu_rlc_span_layout.argtypes = [v, v, u32, C.POINTER(u32), C.POINTER(u32), v]
    if hasattr(L, "fecgpu_rlc_span_one_launch_calls"):  # an older build (PQUIC_AMD_LIB, A/B baselines) lacks it
        L.fecgpu_rlc_span_one_launch_calls.argtypes = []
        L.fecgpu_rlc_span_one_launch_calls.restype = u64
    if hasattr(L, "fecgpu_rlc_window_encode_table"):
        L.fecgpu_rlc_window_encode_table.argtypes = [v, u64, v, u64, u32, u32, u32, v, v]
    if not private:
        _lib = L
    return L


def _addr(x):
    if x is None:
        return None
    if isinstance(x, int):
        return x
    if hasattr(x, "data_ptr"):
        return x.data_ptr()
    return x.ctypes.data  # numpy (host-resident path)


def span_layout(first_id, nss):
    """fecgpu_rlc_span_layout (host only): the received repairs' window starts and lengths -> (base_id, K,
    off), the span's first symbol id, its width and every repair's first column (numpy u8).  Ids may wrap
    modulo 2^32; raises FecGpuError when there is no repair or the windows span more than 128 symbols."""
    import numpy as np
    L = load_library()
    ids = np.ascontiguousarray(first_id, dtype=np.uint32)
    n = np.ascontiguousarray(nss, dtype=np.uint8)
    if ids.shape != n.shape or ids.ndim != 1:
        raise ValueError("span_layout: first_id and nss must be one-dimensional and of one length")
    off = np.zeros(max(len(ids), 1), np.uint8)
    base, K = C.c_uint32(0), C.c_uint32(0)
    rc = L.fecgpu_rlc_span_layout(ids.ctypes.data, n.ctypes.data, len(ids), C.byref(base), C.byref(K),
                                  off.ctypes.data)
    if rc != OK:
        raise FecGpuError(f"fecgpu_rlc_span_layout failed ({rc}): {L.fecgpu_last_error().decode()}")
    return base.value, K.value, off[:len(ids)]


def window_classes(wlen, kmax: int, symbol_size: int):
    """fecgpu_rlc_window_classes (host only): the windows' lengths (1..kmax) -> (perm, first, cnt, len, cchunk,
    nchunks), a stable counting sort by length and the classes' tables cut to the classes present (numpy u32):
    class x holds cnt[x] windows of len[x] symbols from sorted position first[x], its 2 KiB chunks begin at
    chunk cchunk[x]; nchunks is their total.  Raises FecGpuError for a length outside 1..kmax or kmax outside
    1..128."""
    import numpy as np
    L = load_library()
    n = np.ascontiguousarray(wlen, dtype=np.uint8)
    if n.ndim != 1:
        raise ValueError("window_classes: wlen must be one-dimensional")
    perm = np.zeros(max(len(n), 1), np.uint32)
    cls = np.zeros(4 * max(min(int(kmax), 128), 1), np.uint32)
    nc, nch = C.c_uint32(0), C.c_uint64(0)
    rc = L.fecgpu_rlc_window_classes(n.ctypes.data, len(n), kmax, symbol_size, perm.ctypes.data, cls.ctypes.data,
                                     C.byref(nc), C.byref(nch))
    if rc != OK:
        raise FecGpuError(f"fecgpu_rlc_window_classes failed ({rc}): {L.fecgpu_last_error().decode()}")
    t = cls.reshape(4, -1)[:, :nc.value]
    return perm[:len(n)], t[0].copy(), t[1].copy(), t[2].copy(), t[3].copy(), nch.value


def span_one_launch_calls(lib=None) -> int:
    """fecgpu_rlc_span_one_launch_calls (host only): the span decode calls of this process that ran as one
    launch (fecgpu_rlc_span_decode_rows_fused with at most 64 spans, knob plan 0 and a shape that fits LDS)."""
    return int((lib or load_library()).fecgpu_rlc_span_one_launch_calls())


class Engine:
    """Batched FEC engine on one device.  Mirrors fecgpu_* one to one."""

    def __init__(self, device: int = 0, lib_path: str | None = None):
        import torch
        self.torch = torch
        self.lib = load_library(lib_path, private=True) if lib_path else load_library()
        self.device = device
        rc = self.lib.fecgpu_init(device)
        if rc != OK:
            raise FecGpuError(f"fecgpu_init({device}) = {rc}: {self.err()}")

    # ------------------------------------------------------------------ helpers
    def err(self) -> str:
        return self.lib.fecgpu_last_error().decode()

    def version(self) -> str:
        return self.lib.fecgpu_version().decode()

    def _stream(self, stream):
        if stream is None:
            stream = self.torch.cuda.current_stream(self.device)
        return C.c_void_p(stream.cuda_stream if hasattr(stream, "cuda_stream") else int(stream))

    def _check(self, rc, what):
        if rc != OK:
            raise FecGpuError(f"{what} failed ({rc}): {self.err()}")

    def span_one_launch_calls(self) -> int:
        """fecgpu_rlc_span_one_launch_calls of this engine's library."""
        return span_one_launch_calls(self.lib)

    def get_knob(self, name: str) -> int:
        v = C.c_int(0)
        self._check(self.lib.fecgpu_get_knob(name.encode(), C.byref(v)), f"fecgpu_get_knob({name})")
        return v.value

    def set_knob(self, name: str, value: int):
        self._check(self.lib.fecgpu_set_knob(name.encode(), int(value)), f"fecgpu_set_knob({name})")

    def knob(self, name: str, value: int):
        """Context manager: an experiment knob (fecgpu_set_knob) set for the duration of a block."""
        import contextlib

        @contextlib.contextmanager
        def cm():
            old = self.get_knob(name)
            self.set_knob(name, value)
            try:
                yield
            finally:
                self.set_knob(name, old)
        return cm()

    def stats(self) -> dict:
        s = FecGpuStats()
        self.lib.fecgpu_get_stats(C.byref(s))
        return {f: getattr(s, f) for f, _ in s._fields_}

    # ------------------------------------------------------------------ encode
    def rlc_encode(self, src, rep, k: int, r: int, L: int, nblocks: int | None = None,
                   fbn_base: int = 0, fbn=None, stream=None):
        nb = nblocks if nblocks is not None else src.numel() // (k * L)
        self._check(self.lib.fecgpu_rlc_encode(_addr(src), _addr(rep), nb, k, r, L, fbn_base,
                                               _addr(fbn), self._stream(stream)), "fecgpu_rlc_encode")
        return rep

    def rlc_window_encode(self, symbols, rep, nwindows: int, step: int, k: int, r: int, L: int, stream=None):
        """Sliding-window encode: window w = symbols[w*step : w*step + k], block number 0."""
        self._check(self.lib.fecgpu_rlc_window_encode(_addr(symbols), nwindows, step, k, r, L, _addr(rep),
                                                      self._stream(stream)), "fecgpu_rlc_window_encode")
        return rep

    def rlc_window_encode_table(self, symbols, nrows: int, wrow, rep, nwindows: int, k: int, r: int, L: int,
                                stream=None):
        """fecgpu_rlc_window_encode_table: window w = rows wrow[w] .. wrow[w] + k - 1 of a packed stream of
        nrows rows (wrow: u32 device array), block number 0; L % 16 == 0."""
        self._check(self.lib.fecgpu_rlc_window_encode_table(_addr(symbols), nrows, _addr(wrow), nwindows, k, r, L,
                                                            _addr(rep), self._stream(stream)),
                    "fecgpu_rlc_window_encode_table")
        return rep

    def window_rows_workspace_bytes(self, nrows: int, L: int) -> int:
        return int(self.lib.fecgpu_rlc_window_rows_workspace(nrows, L))

    def rlc_window_encode_rows(self, rows, row_len, nrows: int, wrow, rep_rows, blk_len, nwindows: int, k: int,
                               r: int, L: int, workspace=None, stream=None):
        """fecgpu_rlc_window_encode_rows: stream rows by address and length (u64 / u32 device arrays), window w
        = rows wrow[w] .. wrow[w] + k - 1; repair row rep_rows[w*r+i] receives exactly blk_len[w] bytes."""
        if workspace is None:
            n = self.window_rows_workspace_bytes(nrows, L)
            workspace = self.torch.empty(max(n, 16), dtype=self.torch.uint8, device=f"cuda:{self.device}")
        self._check(self.lib.fecgpu_rlc_window_encode_rows(
            _addr(rows), _addr(row_len), nrows, _addr(wrow), _addr(rep_rows), _addr(blk_len), nwindows, k, r, L,
            _addr(workspace), workspace.numel(), self._stream(stream)), "fecgpu_rlc_window_encode_rows")

    def write_repair_frames(self, rep, frames, nblocks: int, r: int, L: int, data_length: int, frame_stride: int,
                            nss: int, nrs: int, fbn_base: int = 0, fbn=None, stream=None):
        """FEC frames (header + payload) for every repair of a batch, on the device."""
        self._check(self.lib.fecgpu_write_repair_frames(_addr(rep), nblocks, r, L, data_length, fbn_base, _addr(fbn),
                                                        nss, nrs, _addr(frames), frame_stride, self._stream(stream)),
                    "fecgpu_write_repair_frames")
        return frames

    def xor_encode(self, src, rep, k: int, L: int, nblocks: int | None = None, stream=None):
        nb = nblocks if nblocks is not None else src.numel() // (k * L)
        self._check(self.lib.fecgpu_xor_encode(_addr(src), _addr(rep), nb, k, L, self._stream(stream)),
                    "fecgpu_xor_encode")
        return rep

    # ------------------------------------------------------------------ decode
    def decode_workspace_bytes(self, nblocks: int, k: int, r: int) -> int:
        return int(self.lib.fecgpu_rlc_decode_workspace(nblocks, k, r))

    def alloc_workspace(self, nblocks: int, k: int, r: int):
        n = self.decode_workspace_bytes(nblocks, k, r)
        return self.torch.empty(max(n, 16), dtype=self.torch.uint8, device=f"cuda:{self.device}")

    def rlc_decode(self, src, rep, src_present, rep_present, status, recovered, k: int, r: int,
                   L: int, nblocks: int | None = None, fbn_base: int = 0, fbn=None,
                   workspace=None, stream=None):
        nb = nblocks if nblocks is not None else src.numel() // (k * L)
        if workspace is None:
            workspace = self.alloc_workspace(nb, k, r)
        self._check(self.lib.fecgpu_rlc_decode(
            _addr(src), _addr(rep), nb, k, r, L, fbn_base, _addr(fbn), _addr(src_present),
            _addr(rep_present), _addr(status), _addr(recovered), _addr(workspace),
            workspace.numel(), self._stream(stream)), "fecgpu_rlc_decode")
        return status, recovered

    def rlc_decode_seeded(self, src, rep, rep_seed, src_present, rep_present, status, recovered, k: int, r: int,
                          L: int, nblocks: int | None = None, workspace=None, stream=None):
        """fecgpu_rlc_decode_seeded: every received repair's coefficients seeded by its own FPID,
        rep_seed[b * r + i] (u32 device array) -- the sliding-window framework's blocks."""
        nb = nblocks if nblocks is not None else src.numel() // (k * L)
        if workspace is None:
            workspace = self.alloc_workspace(nb, k, r)
        self._check(self.lib.fecgpu_rlc_decode_seeded(
            _addr(src), _addr(rep), nb, k, r, L, _addr(rep_seed), _addr(src_present), _addr(rep_present),
            _addr(status), _addr(recovered), _addr(workspace), workspace.numel(), self._stream(stream)),
            "fecgpu_rlc_decode_seeded")
        return status, recovered

    def rlc_decode_full(self, src, rep, src_present, rep_present, status, recovered, k: int, r: int,
                        L: int, nblocks: int | None = None, fbn_base: int = 0, fbn=None, rep_seed=None,
                        workspace=None, stream=None):
        """fecgpu_rlc_decode_full: full-rank mode -- every block the received symbols determine is
        recovered (BLOCK_RECOVERED), the others are BLOCK_SINGULAR; never BLOCK_REF_UB.  rep_seed (u32
        device array [nblocks][r]) selects the seeded form, else (fbn << 8) | i from fbn / fbn_base."""
        nb = nblocks if nblocks is not None else src.numel() // (k * L)
        if workspace is None:
            workspace = self.alloc_workspace(nb, k, r)
        self._check(self.lib.fecgpu_rlc_decode_full(
            _addr(src), _addr(rep), nb, k, r, L, fbn_base, _addr(fbn), _addr(rep_seed), _addr(src_present),
            _addr(rep_present), _addr(status), _addr(recovered), _addr(workspace), workspace.numel(),
            self._stream(stream)), "fecgpu_rlc_decode_full")
        return status, recovered

    def rlc_decode_plan_full(self, src_present, rep_present, k, r, nblocks, workspace, fbn_base=0, fbn=None,
                             rep_seed=None, stream=None):
        """fecgpu_rlc_decode_plan_full: full-rank mode's plan; pairs with rlc_decode_apply, _apply_to and
        _apply_packed."""
        self._check(self.lib.fecgpu_rlc_decode_plan_full(nblocks, k, r, fbn_base, _addr(fbn), _addr(rep_seed),
                                                         _addr(src_present), _addr(rep_present), _addr(workspace),
                                                         workspace.numel(), self._stream(stream)),
                    "fecgpu_rlc_decode_plan_full")

    def rlc_span_decode_plan(self, rep_seed, rep_off, rep_nss, src_present, rep_present, K, R, nspans, workspace,
                             stream=None):
        """fecgpu_rlc_span_decode_plan: the span decode's plan (rep_off / rep_nss: u8 device arrays
        [nspans][R]); pairs with rlc_decode_apply, _apply_to and _apply_packed."""
        self._check(self.lib.fecgpu_rlc_span_decode_plan(nspans, K, R, _addr(rep_seed), _addr(rep_off),
                                                         _addr(rep_nss), _addr(src_present), _addr(rep_present),
                                                         _addr(workspace), workspace.numel(), self._stream(stream)),
                    "fecgpu_rlc_span_decode_plan")

    def rlc_span_decode(self, src, rep, rep_seed, rep_off, rep_nss, src_present, rep_present, status, recovered,
                        K: int, R: int, L: int, nspans: int | None = None, workspace=None, stream=None):
        """fecgpu_rlc_span_decode: the joint decode of overlapping windows -- every missing source the received
        repairs of the span determine is recovered in place, also when the whole span is not determined."""
        nb = nspans if nspans is not None else src.numel() // (K * L)
        if workspace is None:
            workspace = self.alloc_workspace(nb, K, R)
        self._check(self.lib.fecgpu_rlc_span_decode(
            _addr(src), _addr(rep), nb, K, R, L, _addr(rep_seed), _addr(rep_off), _addr(rep_nss),
            _addr(src_present), _addr(rep_present), _addr(status), _addr(recovered), _addr(workspace),
            workspace.numel(), self._stream(stream)), "fecgpu_rlc_span_decode")
        return status, recovered

    def rlc_span_decode_rows_fused(self, src_rows, src_len, rep_rows, rep_len, blk_len, rep_seed, rep_off, rep_nss,
                                   src_present, rep_present, status, recovered, nspans: int, K: int, R: int, L: int,
                                   workspace=None, stream=None):
        """fecgpu_rlc_span_decode_rows_fused: the span decode on rows by address with a length each; every
        determined source receives exactly blk_len[b] bytes."""
        if workspace is None:
            workspace = self.alloc_workspace(nspans, K, R)
        self._check(self.lib.fecgpu_rlc_span_decode_rows_fused(
            _addr(src_rows), _addr(src_len), _addr(rep_rows), _addr(rep_len), _addr(blk_len), nspans, K, R, L,
            _addr(rep_seed), _addr(rep_off), _addr(rep_nss), _addr(src_present), _addr(rep_present),
            _addr(status), _addr(recovered), _addr(workspace), workspace.numel(), self._stream(stream)),
            "fecgpu_rlc_span_decode_rows_fused")
        return status, recovered

    def rlc_decode_stages(self, src, rep, src_present, rep_present, status, recovered, k, r, L, nblocks,
                          workspace, fbn_base=0, stream=None, events=None, dst=None, packed=False):
        """fecgpu_rlc_decode as its two stages (plan, apply); events[i] (if given) recorded before
        stage i and events[2] after the last, on the launch stream.  dst: write the recovered rows
        there (src's layout, fecgpu_rlc_decode_apply_to; packed=True: [nblocks][min(k, r)] rows,
        fecgpu_rlc_decode_apply_packed) instead of into src."""
        st = self._stream(stream)
        torch_stream = stream if stream is not None else self.torch.cuda.current_stream(self.device)
        rec = (lambda i: events[i].record(torch_stream)) if events else (lambda i: None)
        rec(0)
        self._check(self.lib.fecgpu_rlc_decode_plan(nblocks, k, r, fbn_base, None, _addr(src_present),
                                                    _addr(rep_present), _addr(workspace), workspace.numel(), st),
                    "fecgpu_rlc_decode_plan")
        rec(1)
        if dst is not None and packed:
            self._check(self.lib.fecgpu_rlc_decode_apply_packed(_addr(src), _addr(rep), _addr(dst), nblocks, k, r,
                                                                L, _addr(status), _addr(recovered),
                                                                _addr(workspace), workspace.numel(), st),
                        "fecgpu_rlc_decode_apply_packed")
        elif dst is None:
            self._check(self.lib.fecgpu_rlc_decode_apply(_addr(src), _addr(rep), nblocks, k, r, L, _addr(status),
                                                         _addr(recovered), _addr(workspace), workspace.numel(), st),
                        "fecgpu_rlc_decode_apply")
        else:
            self._check(self.lib.fecgpu_rlc_decode_apply_to(_addr(src), _addr(rep), _addr(dst), nblocks, k, r, L,
                                                            _addr(status), _addr(recovered), _addr(workspace),
                                                            workspace.numel(), st), "fecgpu_rlc_decode_apply_to")
        rec(2)
        return status, recovered

    def rlc_decode_plan(self, src_present, rep_present, k, r, nblocks, workspace, fbn_base=0, fbn=None,
                        stream=None):
        """fecgpu_rlc_decode_plan: coefficient-only stage (needs only the presence masks)."""
        self._check(self.lib.fecgpu_rlc_decode_plan(nblocks, k, r, fbn_base, _addr(fbn), _addr(src_present),
                                                    _addr(rep_present), _addr(workspace), workspace.numel(),
                                                    self._stream(stream)), "fecgpu_rlc_decode_plan")

    def rlc_decode_apply(self, src, rep, status, recovered, k, r, L, nblocks, workspace, stream=None):
        """fecgpu_rlc_decode_apply: the data pass plus the zero/undetermined rule."""
        self._check(self.lib.fecgpu_rlc_decode_apply(_addr(src), _addr(rep), nblocks, k, r, L, _addr(status),
                                                     _addr(recovered), _addr(workspace), workspace.numel(),
                                                     self._stream(stream)), "fecgpu_rlc_decode_apply")
        return status, recovered

    def rlc_decode_apply_to(self, src, rep, dst, status, recovered, k, r, L, nblocks, workspace, stream=None):
        """fecgpu_rlc_decode_apply_to: as apply, recovered symbols written to dst (src's layout)."""
        self._check(self.lib.fecgpu_rlc_decode_apply_to(_addr(src), _addr(rep), _addr(dst), nblocks, k, r, L,
                                                        _addr(status), _addr(recovered), _addr(workspace),
                                                        workspace.numel(), self._stream(stream)),
                    "fecgpu_rlc_decode_apply_to")
        return status, recovered

    def rlc_decode_apply_packed(self, src, rep, dst, status, recovered, k, r, L, nblocks, workspace, stream=None):
        """fecgpu_rlc_decode_apply_packed: as apply, recovered symbols packed into dst [nblocks][min(k, r)][L]
        (row u = the u-th missing source of the block, ascending)."""
        self._check(self.lib.fecgpu_rlc_decode_apply_packed(_addr(src), _addr(rep), _addr(dst), nblocks, k, r, L,
                                                            _addr(status), _addr(recovered), _addr(workspace),
                                                            workspace.numel(), self._stream(stream)),
                    "fecgpu_rlc_decode_apply_packed")
        return status, recovered

    def xor_decode(self, src, rep, src_present, rep_present, status, recovered, k: int, L: int,
                   nblocks: int | None = None, stream=None):
        nb = nblocks if nblocks is not None else src.numel() // (k * L)
        self._check(self.lib.fecgpu_xor_decode(_addr(src), _addr(rep), nb, k, L, _addr(src_present),
                                               _addr(rep_present), _addr(status), _addr(recovered),
                                               self._stream(stream)), "fecgpu_xor_decode")
        return status, recovered

    def xor_decode_to(self, src, rep, dst, src_present, rep_present, status, recovered, k: int, L: int,
                      nblocks: int | None = None, stream=None):
        """fecgpu_xor_decode_to: the recovered symbol of block b into dst[b] (one row per block); src is read only."""
        nb = nblocks if nblocks is not None else src.numel() // (k * L)
        self._check(self.lib.fecgpu_xor_decode_to(_addr(src), _addr(rep), _addr(dst), nb, k, L, _addr(src_present),
                                                  _addr(rep_present), _addr(status), _addr(recovered),
                                                  self._stream(stream)), "fecgpu_xor_decode_to")
        return status, recovered

    # ------------------------------------------------------------------ ragged rows
    def rows_gather(self, rows, lens, nrows: int, L: int, dst, stream=None):
        """fecgpu_rows_gather: row x (address rows[x], u64; lens[x] bytes, u32) -> dst[x], zero-padded to L."""
        self._check(self.lib.fecgpu_rows_gather(_addr(rows), _addr(lens), nrows, L, _addr(dst),
                                                self._stream(stream)), "fecgpu_rows_gather")
        return dst

    def rows_scatter(self, src, rows, lens, nrows: int, L: int, stream=None):
        """fecgpu_rows_scatter: lens[x] bytes of packed row src[x] -> address rows[x], not a byte more."""
        self._check(self.lib.fecgpu_rows_scatter(_addr(src), _addr(rows), _addr(lens), nrows, L,
                                                 self._stream(stream)), "fecgpu_rows_scatter")

    def rows_len_workspace_bytes(self, nblocks: int, k: int, r: int, L: int) -> int:
        return int(self.lib.fecgpu_rlc_rows_len_workspace(nblocks, k, r, L))

    def alloc_rows_len_workspace(self, nblocks: int, k: int, r: int, L: int):
        n = self.rows_len_workspace_bytes(nblocks, k, r, L)
        return self.torch.empty(max(n, 16), dtype=self.torch.uint8, device=f"cuda:{self.device}")

    def rlc_encode_rows(self, src_rows, rep_rows, nblocks: int, k: int, r: int, L: int, fbn_base: int = 0,
                        fbn=None, stream=None):
        """fecgpu_rlc_encode_rows: every row of L bytes given by its device address (u64 tables)."""
        self._check(self.lib.fecgpu_rlc_encode_rows(_addr(src_rows), _addr(rep_rows), nblocks, k, r, L, fbn_base,
                                                    _addr(fbn), self._stream(stream)), "fecgpu_rlc_encode_rows")

    def rlc_encode_rows_len(self, src_rows, src_len, rep_rows, blk_len, nblocks: int, k: int, r: int, L: int,
                            fbn_base: int = 0, fbn=None, workspace=None, stream=None):
        """fecgpu_rlc_encode_rows_len: ragged rows -- src_len[b*k+j] <= blk_len[b] <= L (u32 device arrays);
        every repair row receives exactly blk_len[b] bytes."""
        if workspace is None:
            workspace = self.alloc_rows_len_workspace(nblocks, k, r, L)
        self._check(self.lib.fecgpu_rlc_encode_rows_len(
            _addr(src_rows), _addr(src_len), _addr(rep_rows), _addr(blk_len), nblocks, k, r, L, fbn_base,
            _addr(fbn), _addr(workspace), workspace.numel(), self._stream(stream)), "fecgpu_rlc_encode_rows_len")

    def rlc_decode_rows_len(self, src_rows, src_len, rep_rows, rep_len, blk_len, rep_seed, src_present,
                            rep_present, status, recovered, nblocks: int, k: int, r: int, L: int,
                            workspace=None, stream=None):
        """fecgpu_rlc_decode_rows_len: ragged rows, per-repair seeds; every missing source whose recovered
        bit is set receives exactly blk_len[b] bytes at src_rows[b*k+j]."""
        if workspace is None:
            workspace = self.alloc_rows_len_workspace(nblocks, k, r, L)
        self._check(self.lib.fecgpu_rlc_decode_rows_len(
            _addr(src_rows), _addr(src_len), _addr(rep_rows), _addr(rep_len), _addr(blk_len), nblocks, k, r, L,
            _addr(rep_seed), _addr(src_present), _addr(rep_present), _addr(status), _addr(recovered),
            _addr(workspace), workspace.numel(), self._stream(stream)), "fecgpu_rlc_decode_rows_len")
        return status, recovered

    def rlc_encode_rows_fused(self, src_rows, src_len, rep_rows, blk_len, nblocks: int, k: int, r: int, L: int,
                              fbn_base: int = 0, fbn=None, stream=None):
        """fecgpu_rlc_encode_rows_fused: ragged rows in one pass, no workspace; every repair row receives
        exactly blk_len[b] bytes."""
        self._check(self.lib.fecgpu_rlc_encode_rows_fused(
            _addr(src_rows), _addr(src_len), _addr(rep_rows), _addr(blk_len), nblocks, k, r, L, fbn_base,
            _addr(fbn), self._stream(stream)), "fecgpu_rlc_encode_rows_fused")

    def rlc_decode_rows_fused(self, src_rows, src_len, rep_rows, rep_len, blk_len, rep_seed, src_present,
                              rep_present, status, recovered, nblocks: int, k: int, r: int, L: int,
                              workspace=None, stream=None):
        """fecgpu_rlc_decode_rows_fused: ragged rows in one pass, per-repair seeds; the workspace is the plan's
        (decode_workspace_bytes).  Every missing source whose recovered bit is set holds its blk_len[b] bytes."""
        if workspace is None:
            workspace = self.alloc_workspace(nblocks, k, r)
        self._check(self.lib.fecgpu_rlc_decode_rows_fused(
            _addr(src_rows), _addr(src_len), _addr(rep_rows), _addr(rep_len), _addr(blk_len), nblocks, k, r, L,
            _addr(rep_seed), _addr(src_present), _addr(rep_present), _addr(status), _addr(recovered),
            _addr(workspace), workspace.numel(), self._stream(stream)), "fecgpu_rlc_decode_rows_fused")
        return status, recovered

    def rlc_decode_rows_full(self, src_rows, rep_rows, rep_seed, src_present, rep_present, status, recovered,
                             nblocks: int, k: int, r: int, L: int, workspace=None, stream=None):
        """fecgpu_rlc_decode_rows_full: rows by address in full-rank mode (status RECOVERED or SINGULAR, never
        REF_UB); a repair full mode does not select is never dereferenced."""
        if workspace is None:
            workspace = self.alloc_workspace(nblocks, k, r)
        self._check(self.lib.fecgpu_rlc_decode_rows_full(
            _addr(src_rows), _addr(rep_rows), nblocks, k, r, L, _addr(rep_seed), _addr(src_present),
            _addr(rep_present), _addr(status), _addr(recovered), _addr(workspace), workspace.numel(),
            self._stream(stream)), "fecgpu_rlc_decode_rows_full")
        return status, recovered

    def rlc_decode_rows_fused_full(self, src_rows, src_len, rep_rows, rep_len, blk_len, rep_seed, src_present,
                                   rep_present, status, recovered, nblocks: int, k: int, r: int, L: int,
                                   workspace=None, stream=None):
        """fecgpu_rlc_decode_rows_fused_full: rlc_decode_rows_fused in full-rank mode."""
        if workspace is None:
            workspace = self.alloc_workspace(nblocks, k, r)
        self._check(self.lib.fecgpu_rlc_decode_rows_fused_full(
            _addr(src_rows), _addr(src_len), _addr(rep_rows), _addr(rep_len), _addr(blk_len), nblocks, k, r, L,
            _addr(rep_seed), _addr(src_present), _addr(rep_present), _addr(status), _addr(recovered),
            _addr(workspace), workspace.numel(), self._stream(stream)), "fecgpu_rlc_decode_rows_fused_full")
        return status, recovered

    def xor_encode_rows(self, src_rows, src_len, rep_rows, blk_len, nblocks: int, k: int, L: int, stream=None):
        """fecgpu_xor_encode_rows: one pass over rows given by address (u64 tables) and length (u32);
        rep_rows[b] receives exactly blk_len[b] bytes."""
        self._check(self.lib.fecgpu_xor_encode_rows(_addr(src_rows), _addr(src_len), _addr(rep_rows),
                                                    _addr(blk_len), nblocks, k, L, self._stream(stream)),
                    "fecgpu_xor_encode_rows")

    def xor_decode_rows(self, src_rows, src_len, rep_rows, blk_len, src_present, rep_present, status, recovered,
                        nblocks: int, k: int, L: int, stream=None):
        """fecgpu_xor_decode_rows: the missing source of a RECOVERED block receives exactly blk_len[b] bytes at
        its own row, src_rows[b*k+miss]."""
        self._check(self.lib.fecgpu_xor_decode_rows(_addr(src_rows), _addr(src_len), _addr(rep_rows),
                                                    _addr(blk_len), nblocks, k, L, _addr(src_present),
                                                    _addr(rep_present), _addr(status), _addr(recovered),
                                                    self._stream(stream)), "fecgpu_xor_decode_rows")
        return status, recovered

    def synth_fill(self, dst, nbytes: int, seed: int, offset: int = 0, stream=None):
        self._check(self.lib.fecgpu_synth_fill(_addr(dst), nbytes, seed, offset, self._stream(stream)),
                    "fecgpu_synth_fill")
        return dst


class HostPath:
    """Host-resident entry points (include/fecgpu.h 'Host-resident path'): host buffers in,
    host buffers out, H2D/D2H overlapped with the kernels on `nstreams` streams."""

    def __init__(self, device: int = 0, nstreams: int = 3, chunk_bytes: int = 64 << 20):
        self.lib = load_library()
        self.ctx = self.lib.fecgpu_host_ctx_create(device, nstreams, chunk_bytes)
        if not self.ctx:
            raise FecGpuError(f"fecgpu_host_ctx_create({device}) failed: {self.lib.fecgpu_last_error().decode()}")

    def close(self):
        if self.ctx:
            self.lib.fecgpu_host_ctx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        if rc != OK:
            raise FecGpuError(f"{what} failed ({rc}): {self.lib.fecgpu_last_error().decode()}")

    def rlc_encode(self, src, rep, nblocks, k, r, L, fbn_base=0):
        self._chk(self.lib.fecgpu_rlc_encode_host(self.ctx, _addr(src), _addr(rep), nblocks, k, r, L, fbn_base,
                                                  None), "fecgpu_rlc_encode_host")

    def rlc_window_encode(self, symbols, nrows, wrow, rep, nwindows, k, r, L):
        """fecgpu_rlc_window_encode_host: window w = rows wrow[w] .. wrow[w] + k of the stream (wrow: host u32)."""
        self._chk(self.lib.fecgpu_rlc_window_encode_host(self.ctx, _addr(symbols), nrows, _addr(wrow), nwindows, k, r,
                                                         L, _addr(rep)), "fecgpu_rlc_window_encode_host")

    def rlc_decode(self, src, rep, sp, rp, status, rec, nblocks, k, r, L, fbn_base=0):
        self._chk(self.lib.fecgpu_rlc_decode_host(self.ctx, _addr(src), _addr(rep), nblocks, k, r, L, fbn_base,
                                                  None, _addr(sp), _addr(rp), _addr(status), _addr(rec)),
                  "fecgpu_rlc_decode_host")

    def rlc_decode_seeded(self, src, rep, seeds, sp, rp, status, rec, nblocks, k, r, L):
        self._chk(self.lib.fecgpu_rlc_decode_host_seeded(self.ctx, _addr(src), _addr(rep), nblocks, k, r, L,
                                                         _addr(seeds), _addr(sp), _addr(rp), _addr(status),
                                                         _addr(rec)), "fecgpu_rlc_decode_host_seeded")

    def rlc_decode_full(self, src, rep, sp, rp, status, rec, nblocks, k, r, L, fbn_base=0, fbn=None, seeds=None):
        """fecgpu_rlc_decode_host_full: full-rank mode on host buffers (fbn / seeds: host arrays)."""
        self._chk(self.lib.fecgpu_rlc_decode_host_full(self.ctx, _addr(src), _addr(rep), nblocks, k, r, L, fbn_base,
                                                       _addr(fbn), _addr(seeds), _addr(sp), _addr(rp),
                                                       _addr(status), _addr(rec)), "fecgpu_rlc_decode_host_full")

    def rlc_encode_rows_len(self, src_rows, src_len, rep_rows, blk_len, nblocks, k, r, L, fbn=None):
        """fecgpu_rlc_encode_rows_len_host: host tables and lengths; the rows must be device-accessible."""
        self._chk(self.lib.fecgpu_rlc_encode_rows_len_host(self.ctx, _addr(src_rows), _addr(src_len),
                                                           _addr(rep_rows), _addr(blk_len), nblocks, k, r, L,
                                                           _addr(fbn)), "fecgpu_rlc_encode_rows_len_host")

    def rlc_decode_rows_len(self, src_rows, src_len, rep_rows, rep_len, blk_len, seeds, sp, rp, status, rec,
                            nblocks, k, r, L):
        """fecgpu_rlc_decode_rows_len_host: host tables, lengths, seeds, masks, status and recovered."""
        self._chk(self.lib.fecgpu_rlc_decode_rows_len_host(self.ctx, _addr(src_rows), _addr(src_len),
                                                           _addr(rep_rows), _addr(rep_len), _addr(blk_len),
                                                           nblocks, k, r, L, _addr(seeds), _addr(sp), _addr(rp),
                                                           _addr(status), _addr(rec)),
                  "fecgpu_rlc_decode_rows_len_host")

    def rlc_encode_rows_fused(self, src_rows, src_len, rep_rows, blk_len, nblocks, k, r, L, fbn=None):
        """fecgpu_rlc_encode_rows_fused_host: host tables and lengths; the rows must be device-accessible."""
        self._chk(self.lib.fecgpu_rlc_encode_rows_fused_host(self.ctx, _addr(src_rows), _addr(src_len),
                                                             _addr(rep_rows), _addr(blk_len), nblocks, k, r, L,
                                                             _addr(fbn)), "fecgpu_rlc_encode_rows_fused_host")

    def rlc_decode_rows_fused(self, src_rows, src_len, rep_rows, rep_len, blk_len, seeds, sp, rp, status, rec,
                              nblocks, k, r, L):
        """fecgpu_rlc_decode_rows_fused_host: host tables, lengths, seeds, masks, status and recovered."""
        self._chk(self.lib.fecgpu_rlc_decode_rows_fused_host(self.ctx, _addr(src_rows), _addr(src_len),
                                                             _addr(rep_rows), _addr(rep_len), _addr(blk_len),
                                                             nblocks, k, r, L, _addr(seeds), _addr(sp), _addr(rp),
                                                             _addr(status), _addr(rec)),
                  "fecgpu_rlc_decode_rows_fused_host")

    def rlc_decode_rows_full(self, src_rows, rep_rows, seeds, sp, rp, status, rec, nblocks, k, r, L):
        """fecgpu_rlc_decode_rows_host_full: host tables, seeds, masks, status and recovered; full-rank mode."""
        self._chk(self.lib.fecgpu_rlc_decode_rows_host_full(self.ctx, _addr(src_rows), _addr(rep_rows), nblocks, k,
                                                            r, L, _addr(seeds), _addr(sp), _addr(rp), _addr(status),
                                                            _addr(rec)), "fecgpu_rlc_decode_rows_host_full")

    def rlc_decode_rows_fused_full(self, src_rows, src_len, rep_rows, rep_len, blk_len, seeds, sp, rp, status, rec,
                                   nblocks, k, r, L):
        """fecgpu_rlc_decode_rows_fused_host_full: rlc_decode_rows_fused in full-rank mode."""
        self._chk(self.lib.fecgpu_rlc_decode_rows_fused_host_full(self.ctx, _addr(src_rows), _addr(src_len),
                                                                  _addr(rep_rows), _addr(rep_len), _addr(blk_len),
                                                                  nblocks, k, r, L, _addr(seeds), _addr(sp),
                                                                  _addr(rp), _addr(status), _addr(rec)),
                  "fecgpu_rlc_decode_rows_fused_host_full")

    def rlc_span_decode_rows_fused(self, src_rows, src_len, rep_rows, rep_len, blk_len, seeds, rep_off, rep_nss, sp,
                                   rp, status, rec, nspans, K, R, L):
        """fecgpu_rlc_span_decode_rows_fused_host: host tables, lengths, seeds, windows, masks, status and
        recovered; the rows must be device-accessible."""
        self._chk(self.lib.fecgpu_rlc_span_decode_rows_fused_host(
            self.ctx, _addr(src_rows), _addr(src_len), _addr(rep_rows), _addr(rep_len), _addr(blk_len), nspans, K,
            R, L, _addr(seeds), _addr(rep_off), _addr(rep_nss), _addr(sp), _addr(rp), _addr(status), _addr(rec)),
            "fecgpu_rlc_span_decode_rows_fused_host")

    def xor_encode_rows(self, src_rows, src_len, rep_rows, blk_len, nblocks, k, L):
        """fecgpu_xor_encode_rows_host: host tables and lengths; the rows must be device-accessible."""
        self._chk(self.lib.fecgpu_xor_encode_rows_host(self.ctx, _addr(src_rows), _addr(src_len), _addr(rep_rows),
                                                       _addr(blk_len), nblocks, k, L), "fecgpu_xor_encode_rows_host")

    def xor_decode_rows(self, src_rows, src_len, rep_rows, blk_len, sp, rp, status, rec, nblocks, k, L):
        """fecgpu_xor_decode_rows_host: host tables, lengths, masks, status and recovered."""
        self._chk(self.lib.fecgpu_xor_decode_rows_host(self.ctx, _addr(src_rows), _addr(src_len), _addr(rep_rows),
                                                       _addr(blk_len), nblocks, k, L, _addr(sp), _addr(rp),
                                                       _addr(status), _addr(rec)), "fecgpu_xor_decode_rows_host")

    def rlc_window_encode_rows(self, rows, row_len, nrows, wrow, rep_rows, blk_len, nwindows, k, r, L):
        """fecgpu_rlc_window_encode_rows_host: host tables (stream rows, lengths, window starts, repair rows,
        window lengths); the rows must be device-accessible."""
        self._chk(self.lib.fecgpu_rlc_window_encode_rows_host(self.ctx, _addr(rows), _addr(row_len), nrows,
                                                              _addr(wrow), _addr(rep_rows), _addr(blk_len),
                                                              nwindows, k, r, L),
                  "fecgpu_rlc_window_encode_rows_host")

    def rlc_window_encode_rows_var(self, rows, row_len, nrows, wrow, wlen, rep_rows, blk_len, nwindows, kmax, r, L):
        """fecgpu_rlc_window_encode_rows_var_host: rlc_window_encode_rows with a length per window (wlen: host
        u8, 1..kmax); window w protects rows wrow[w] .. wrow[w] + wlen[w] - 1."""
        self._chk(self.lib.fecgpu_rlc_window_encode_rows_var_host(self.ctx, _addr(rows), _addr(row_len), nrows,
                                                                  _addr(wrow), _addr(wlen), _addr(rep_rows),
                                                                  _addr(blk_len), nwindows, kmax, r, L),
                  "fecgpu_rlc_window_encode_rows_var_host")
