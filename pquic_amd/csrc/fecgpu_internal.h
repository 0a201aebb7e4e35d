// pquic_amd/csrc/fecgpu_internal.h -- what fec_engine.hip and host_path.hip use of each other.
//
// Library-internal: C linkage, hidden visibility, so none of these is an exported symbol.  Both files
// include this header, and the compiler checks each definition against its declaration.
#ifndef FECGPU_INTERNAL_H
#define FECGPU_INTERNAL_H

#include <stddef.h>
#include <stdint.h>

#define FECGPU_INTERNAL __attribute__((visibility("hidden")))

#ifdef __cplusplus
extern "C" {
#endif

// fec_engine.hip: knob zc_read (page-locked buffers used in place by the kernels; 0: staged copies)
FECGPU_INTERNAL int fecgpu_knob_zc_read(void);
// fec_engine.hip: knob window_sc (which kernel fecgpu_rlc_window_encode_host launches)
FECGPU_INTERNAL int fecgpu_knob_window_sc(void);
// fec_engine.hip: the yield_* knobs of host_path.hip's Pacer
FECGPU_INTERNAL void fecgpu_knob_yield(int *slice_kb, int *depth, int *gate_us, int *streams, int *always,
                                       int *window_ms);
// fec_engine.hip: decode with the recovered rows written to dst; full != 0: full-rank mode
FECGPU_INTERNAL int fecgpu_rlc_decode_to_internal(const void *src, const void *rep, void *dst, uint64_t nblocks,
                                                  uint32_t k, uint32_t r, uint32_t L, uint32_t fbn_base,
                                                  const uint32_t *fbn, const uint32_t *seeds, const uint64_t *sp,
                                                  const uint64_t *rp, uint8_t *status, uint64_t *recovered, void *ws,
                                                  size_t wsb, void *stream, int full);
// fec_engine.hip: fecgpu_rlc_decode_rows / _rows_fused; full != 0: full-rank mode (the *_full forms)
FECGPU_INTERNAL int fecgpu_rlc_decode_rows_internal(const uint64_t *src_rows, const uint64_t *rep_rows, uint64_t nblocks,
                                                    uint32_t k, uint32_t r, uint32_t symbol_size,
                                                    const uint32_t *rep_seed, const uint64_t *src_present,
                                                    const uint64_t *rep_present, uint8_t *status, uint64_t *recovered,
                                                    void *workspace, size_t workspace_bytes, void *stream, int full);
FECGPU_INTERNAL int fecgpu_rlc_decode_rows_fused_internal(
    const uint64_t *src_rows, const uint32_t *src_len, const uint64_t *rep_rows, const uint32_t *rep_len,
    const uint32_t *blk_len, uint64_t nblocks, uint32_t k, uint32_t r, uint32_t symbol_size, const uint32_t *rep_seed,
    const uint64_t *src_present, const uint64_t *rep_present, uint8_t *status, uint64_t *recovered, void *workspace,
    size_t workspace_bytes, void *stream, int full);
// fec_engine.hip: fecgpu_rlc_window_encode_rows on windows of their own length, sorted into classes by
// fecgpu_rlc_window_classes: perm[nwindows], cls[4 * kmax] and nchunks are its outputs, device-accessible
FECGPU_INTERNAL int fecgpu_rlc_window_encode_rows_var_internal(
    const uint64_t *rows, const uint32_t *row_len, uint64_t nrows, const uint32_t *wrow, const uint64_t *rep_rows,
    const uint32_t *blk_len, uint64_t nwindows, uint32_t kmax, uint32_t r, uint32_t symbol_size, const uint32_t *perm,
    const uint32_t *cls, uint64_t nchunks, void *workspace, size_t workspace_bytes, void *stream);
// fec_engine.hip: fecgpu_rlc_encode_rows_len with the packed arrays given one by one
FECGPU_INTERNAL int fecgpu_rlc_encode_rows_len_internal(const uint64_t *src_rows, const uint32_t *src_len,
                                                        const uint64_t *rep_rows, const uint32_t *blk_len,
                                                        uint64_t nblocks, uint32_t k, uint32_t r, uint32_t L,
                                                        uint32_t fbn_base, const uint32_t *fbn, void *psrc, void *prep,
                                                        void *stream);
// fec_engine.hip: fecgpu_rlc_decode_rows_len with the packed arrays and the plan workspace given one by one
FECGPU_INTERNAL int fecgpu_rlc_decode_rows_len_internal(const uint64_t *src_rows, const uint32_t *src_len,
                                                        const uint64_t *rep_rows, const uint32_t *rep_len,
                                                        const uint32_t *blk_len, uint64_t nblocks, uint32_t k,
                                                        uint32_t r, uint32_t L, const uint32_t *rep_seed,
                                                        const uint64_t *sp, const uint64_t *rp, uint8_t *status,
                                                        uint64_t *recovered, void *psrc, void *prep, void *prec,
                                                        void *ws, size_t wsb, void *stream);
// fec_engine.hip: sets the message fecgpu_last_error() returns; returns code
FECGPU_INTERNAL int fecgpu_set_error_internal(int code, const char *what);
// fec_engine.hip: hook requests in flight across every block service of the process
FECGPU_INTERNAL int fecgpu_svc_hooks_pending(void);
// fec_engine.hip: monotonic time of the last hook request in microseconds (0: none yet)
FECGPU_INTERNAL uint64_t fecgpu_svc_last_request_us(void);
// host_path.hip: lookups the page-locked registry answered, and those that went to the runtime
FECGPU_INTERNAL void fecgpu_host_registry_stats(uint64_t *hits, uint64_t *misses);
// host_path.hip: slices the Pacer launched, and slices it held back for a pending hook request
FECGPU_INTERNAL void fecgpu_host_yield_stats(uint64_t *slices, uint64_t *waits);

#ifdef __cplusplus
}
#endif

#endif  // FECGPU_INTERNAL_H
