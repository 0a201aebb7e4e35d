/*
 * include/fecgpu.h -- C ABI of the MI355X FEC engine (libpquic_fec.so).
 *
 * Batched, device-resident replacement for the arithmetic inside PQUIC's FEC scheme
 * pluglets (plugins/fec/fec_scheme_protoops/):
 *   fecgpu_rlc_encode  <- fec_generate_repair_symbols, RLC-GF(256)
 *                         (rlc_fec_scheme_generate_gf256.c:24-77)
 *   fecgpu_rlc_decode  <- fec_recover, RLC-GF(256) Gaussian elimination
 *                         (rlc_fec_scheme_gf256.c:134-251)
 *   fecgpu_xor_encode  <- fec_generate_repair_symbols, XOR (xor_fec_scheme_generate.c:41-78)
 *   fecgpu_xor_decode  <- fec_recover, XOR (xor_fec_scheme.c:41-74)
 * The per-block protoop adapters that keep the reference's hook surface are declared in
 * include/pquic_fec_protoops.h and call these entry points.
 *
 * Layout (all device pointers, HBM-resident, 4-byte aligned):
 *   src  [nblocks][k][symbol_size]   source symbols of consecutive FEC blocks
 *   rep  [nblocks][r][symbol_size]   repair symbols
 * Equal-length symbols; symbol_size % 4 == 0 (callers with ragged payloads zero-pad to a
 * common length, which is what the reference does internally: every symbol of a block is
 * treated as zero-padded to max(data_length)).  The *_rows_len entry points ("Ragged rows" below)
 * take a length per row instead and do that padding on the device.
 * FEC block number of block b: fbn[b] if fbn != NULL, else (fbn_base + b) mod 2^24.
 * RLC coefficients of repair i of block fbn come from TinyMT32 seeded with
 * (fbn << 8) | i, exactly as the reference (fec.h:44-75).
 *
 * `stream` is a hipStream_t (NULL = the null stream).  Every call is asynchronous and
 * graph-capturable: no allocation, no synchronisation inside.  Call fecgpu_init(device) before capturing: its
 * once-per-device check (one allocation, one synchronisation) otherwise runs inside the first launch.  The one
 * other first-use step sits behind an experiment knob: with plan = 2 forced, shapes whose lane plan needs more
 * than 64 KiB of LDS raise that kernel's limit (hipFuncSetAttribute) at their first plan call; make it eagerly.
 */
#ifndef PQUIC_FECGPU_H
#define PQUIC_FECGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Call status. */
#define FECGPU_OK              0
#define FECGPU_ERR_INVALID    -1   /* argument out of range / NULL / misaligned          */
#define FECGPU_ERR_HIP        -2   /* a HIP runtime call failed: fecgpu_last_error()     */
#define FECGPU_ERR_NO_DEVICE  -3   /* no gfx950 device visible                           */
#define FECGPU_ERR_NOMEM      -4   /* workspace too small / allocation failed            */

/* Per-block decode outcome written to status[b]. */
#define FECGPU_BLOCK_RECOVERED 0   /* recovery ran (reference fec_recover returned 0 after
                                      solving); recovered[] lists the inserted sources     */
#define FECGPU_BLOCK_NOTHING   1   /* a precondition failed; nothing to recover          */
#define FECGPU_BLOCK_REF_UB    2   /* erasure pattern on which the reference dereferences
                                      x[-1] (rlc_fec_scheme_gf256.c:74-77) or a NULL repair
                                      (xor_fec_scheme.c:50-51): no output, flagged          */
#define FECGPU_BLOCK_SINGULAR  3   /* full-rank mode only (fecgpu_rlc_decode_full): the received
                                      repairs have rank < the number of missing sources, so the
                                      block is not determined: no output, recovered[] = 0     */

#define FECGPU_MAX_K 128           /* presence masks are 2 x u64 per block               */
#define FECGPU_MAX_R 128

/* Engine version / device check.  Returns FECGPU_OK when a gfx950 device is usable. */
int fecgpu_init(int device);
const char *fecgpu_version(void);
const char *fecgpu_last_error(void);

/* RLC-GF(256) encode: rep[b][i] = sum_j coef(fbn_b, i)[j] * src[b][j] over GF(2^8)/0x11D. */
int fecgpu_rlc_encode(const void *src, void *rep, uint64_t nblocks, uint32_t k, uint32_t r,
                      uint32_t symbol_size, uint32_t fbn_base, const uint32_t *fbn,
                      void *stream);

/* Sliding-window RLC encode (window_framework_sender.h:214-250): window w protects the k
 * consecutive symbols starting at symbol w * step of one symbol stream (windows overlap when
 * step < k; symbols[] holds (nwindows - 1) * step + k rows of symbol_size bytes).  Window
 * blocks carry fec_block_number 0 (malloc_fec_block(cnx, 0), :218), so every window's
 * coefficients are seeded by the repair index alone:
 *   rep[w][i] = sum_j coef(0, i)[j] * symbols[w * step + j]. */
int fecgpu_rlc_window_encode(const void *symbols, uint64_t nwindows, uint32_t step, uint32_t k, uint32_t r,
                             uint32_t symbol_size, void *rep, void *stream);

/* Window encode over de-duplicated symbol streams (the batching adapter's window jobs): symbols[] holds
 * nrows rows of symbol_size bytes -- each connection's symbols once, in order -- and window w protects
 * the k rows starting at row wrow[w] (a device array), with block number 0 like every window:
 *   rep[w][i] = sum_j coef(0, i)[j] * symbols[wrow[w] + j].
 * symbol_size % 16 == 0, 16-B aligned buffers, nrows * symbol_size < 2 GiB; knob window_sc != 0.
 * Every window must lie in the stream: wrow[w] + k <= nrows for all w.  wrow[] is device memory, so
 * this entry point cannot check it and the kernel reads the rows it names unchecked (the host form,
 * fecgpu_rlc_window_encode_host, checks it before any launch). */
int fecgpu_rlc_window_encode_table(const void *symbols, uint64_t nrows, const uint32_t *wrow, uint64_t nwindows,
                                   uint32_t k, uint32_t r, uint32_t symbol_size, void *rep, void *stream);

/* Window encode on rows where they lie (the batching adapter's window jobs in registered arenas):
 * rows[x] / row_len[x] are the address and length of stream row x -- each symbol once, in order, as in
 * fecgpu_rlc_window_encode_table -- window w protects rows wrow[w] .. wrow[w] + k - 1 with block number 0,
 * rep_rows[w * r + i] is the address of its repair i and blk_len[w] its length (the reference's
 * max_length).  Repair row (w, i) receives exactly blk_len[w] bytes: the first blk_len[w] bytes
 * fecgpu_rlc_window_encode_table gives on the same rows zero-padded to the width.  Within window w a row
 * counts as zero from min(row_len, blk_len[w]) on: a row longer than one of its windows is truncated for
 * that window only.
 * Two launches: a gather pass lays the stream out once in `workspace` (each row read once, for its own
 * length -- a symbol serves up to k / step windows and crosses the bus once), then the shared-coefficient
 * kernel codes the windows from it and stores every repair straight to its row; there is no packed repair
 * buffer and no scatter pass.
 * Memory rules (those of the *_rows_fused and XOR row forms): row addresses are 4-byte aligned, below
 * 2^48, in device memory or mapped page-locked host memory; a row of 0 bytes is never dereferenced and
 * its address may be 0; a load may touch the aligned dword that holds a row's last byte and nothing after
 * it; stores are 16-B stores, then dword stores, then byte stores for the last 1-3 bytes; no dword is
 * read-modify-written; nothing is written past blk_len[w] bytes of a repair row.  All five tables are
 * device-accessible arrays, so this entry point cannot check them: the kernels clamp blk_len to
 * symbol_size and row_len to the width instead, and trust wrow[w] + k <= nrows (the host form,
 * fecgpu_rlc_window_encode_rows_host, checks all three before any launch).  Asynchronous on `stream`,
 * allocates nothing.
 * symbol_size is a multiple of 4; internally the width is symbol_size rounded up to 16.  workspace: 16-byte
 * aligned device memory of fecgpu_rlc_window_rows_workspace(nrows, symbol_size) bytes (nrows rows of the
 * width).  FECGPU_ERR_INVALID, with a message naming the rule, when (nrows + k) * width reaches 2 GiB (the
 * kernel's 32-bit load offsets) or knob window_sc is 0. */
size_t fecgpu_rlc_window_rows_workspace(uint64_t nrows, uint32_t symbol_size);
int fecgpu_rlc_window_encode_rows(const uint64_t *rows, const uint32_t *row_len, uint64_t nrows,
                                  const uint32_t *wrow, const uint64_t *rep_rows, const uint32_t *blk_len,
                                  uint64_t nwindows, uint32_t k, uint32_t r, uint32_t symbol_size,
                                  void *workspace, size_t workspace_bytes, void *stream);

/* RLC encode with every row given by its address: src_rows[b * k + j] / rep_rows[b * r + i] are the
 * device addresses (4-byte aligned; device memory or mapped page-locked host memory, e.g. a registered
 * plugin arena) of source row j / repair row i of block b, each symbol_size bytes.  The tables and
 * fbn[] must themselves be device-accessible.  Same result as fecgpu_rlc_encode on packed rows. */
int fecgpu_rlc_encode_rows(const uint64_t *src_rows, const uint64_t *rep_rows, uint64_t nblocks, uint32_t k,
                           uint32_t r, uint32_t symbol_size, uint32_t fbn_base, const uint32_t *fbn, void *stream);

/* RLC decode with every row given by its address (the batching adapter's received symbols where they
 * lie in registered plugin arenas): src_rows[b * k + j] is the device address of source row j of block b
 * -- for a received source the row read, for a missing one the row its recovered bytes are written to --
 * and rep_rows[b * r + i] that of repair row i (entries of repairs not present are not read).  Every
 * equation is seeded by rep_seed[b * r + i] (the repair's own FPID, as fecgpu_rlc_decode_seeded); masks,
 * status, recovered and workspace as fecgpu_rlc_decode.  Rows are symbol_size bytes, 4-byte aligned;
 * the tables and arrays must be device-accessible.  Same bytes, status and masks as
 * fecgpu_rlc_decode_seeded on packed rows. */
int fecgpu_rlc_decode_rows(const uint64_t *src_rows, const uint64_t *rep_rows, uint64_t nblocks, uint32_t k,
                           uint32_t r, uint32_t symbol_size, const uint32_t *rep_seed, const uint64_t *src_present,
                           const uint64_t *rep_present, uint8_t *status, uint64_t *recovered, void *workspace,
                           size_t workspace_bytes, void *stream);

/* fecgpu_rlc_decode_rows in full-rank mode: status, recovered and the recovered bytes are those of
 * fecgpu_rlc_decode_full with rep_seed on the packed rows (RECOVERED whenever the received repairs
 * determine the block, SINGULAR otherwise, never REF_UB).  Row rules are fecgpu_rlc_decode_rows's, and one
 * more: a present repair that full mode does not select (it is dependent on earlier ones, or past the
 * n-th independent one) is never dereferenced, like an absent one -- its address may be 0.  A SINGULAR
 * block reads and writes no row. */
int fecgpu_rlc_decode_rows_full(const uint64_t *src_rows, const uint64_t *rep_rows, uint64_t nblocks, uint32_t k,
                                uint32_t r, uint32_t symbol_size, const uint32_t *rep_seed,
                                const uint64_t *src_present, const uint64_t *rep_present, uint8_t *status,
                                uint64_t *recovered, void *workspace, size_t workspace_bytes, void *stream);

/* ---- Ragged rows: symbols of their own length, coded where they lie ------------------------------
 * The reference codes symbols of different lengths: generate reads every source for its own
 * data_length and allocates repairs of the block's max_length (rlc_fec_scheme_generate_gf256.c:41-66);
 * recover takes max_length from the first present repair, reads every received symbol for its own
 * length and allocates recovered sources of max_length (rlc_fec_scheme_gf256.c:186-228).  The entry
 * points below take a length per row beside its address, so a caller pads nothing.
 *
 * fecgpu_rows_gather: row x of the table is copied to dst + x * symbol_size -- len[x] bytes, then zeros
 * up to symbol_size.  fecgpu_rows_scatter: len[x] bytes of packed row x (src + x * symbol_size) go to
 * the row's address, and not one byte more (16-B and dword stores, byte stores for the last 1-3 bytes;
 * no dword is read-modify-written, so the bytes after a row may be written by anyone meanwhile).
 * Row addresses are 4-byte aligned (device memory or mapped page-locked host memory); lengths are any
 * value from 0 to symbol_size.  A row of length 0 is not touched and its address is never dereferenced
 * (it may be 0).  Gather may read the aligned dword that holds a row's last byte (an aligned dword cannot
 * cross a page) and never reads further.  rows[] and len[] are device-accessible arrays, so these entry
 * points cannot check them: the kernels clamp len[x] to symbol_size, so a bad length cannot overrun
 * the packed buffer, and trust the addresses. */
int fecgpu_rows_gather(const uint64_t *rows, const uint32_t *len, uint64_t nrows, uint32_t symbol_size, void *dst,
                       void *stream);
int fecgpu_rows_scatter(const void *src, const uint64_t *rows, const uint32_t *len, uint64_t nrows,
                        uint32_t symbol_size, void *stream);

/* Device scratch of one fecgpu_rlc_encode_rows_len / fecgpu_rlc_decode_rows_len pass over a batch: the
 * packed sources, packed repairs and packed recovered rows ([nblocks][min(k, r)]), each from a 256-B
 * boundary, then fecgpu_rlc_decode_workspace(nblocks, k, r).  16-byte aligned.  Encode uses only the
 * first two arrays and accepts a workspace that ends after them. */
size_t fecgpu_rlc_rows_len_workspace(uint64_t nblocks, uint32_t k, uint32_t r, uint32_t symbol_size);

/* fecgpu_rlc_encode_rows on ragged rows: blk_len[b] <= symbol_size is the length of block b (the
 * reference's max_length) and src_len[b * k + j] <= blk_len[b] that of its source j.  Each repair row
 * receives exactly blk_len[b] bytes: the first blk_len[b] bytes fecgpu_rlc_encode_rows gives on the same
 * rows zero-padded to symbol_size.  Runs gather, fecgpu_rlc_encode on the packed batch, scatter: two
 * more passes over device memory than fecgpu_rlc_encode_rows, which stays the entry point for rows of
 * one length.  src_len[] and blk_len[] are device-accessible arrays, so this entry point cannot check
 * them: the kernels clamp src_len to blk_len and blk_len to symbol_size instead (the host form,
 * fecgpu_rlc_encode_rows_len_host, checks both before any launch). */
int fecgpu_rlc_encode_rows_len(const uint64_t *src_rows, const uint32_t *src_len, const uint64_t *rep_rows,
                               const uint32_t *blk_len, uint64_t nblocks, uint32_t k, uint32_t r,
                               uint32_t symbol_size, uint32_t fbn_base, const uint32_t *fbn, void *workspace,
                               size_t workspace_bytes, void *stream);

/* fecgpu_rlc_decode_rows on ragged rows (reference mode).  A present source / repair is read for
 * min(src_len / rep_len, blk_len[b]) bytes -- a received symbol longer than the block is truncated --
 * and an absent one is not read (its address may be 0 unless it is a missing source to be written).
 * status and recovered are exactly what fecgpu_rlc_decode_seeded gives on the rows zero-padded to
 * symbol_size.  Every missing source whose recovered bit is set receives exactly blk_len[b] bytes at
 * src_rows[b * k + j]; a missing source whose bit stays clear is left alone.  Nothing is ever written
 * past blk_len[b] bytes of a row.  Runs gather (sources, repairs), the plan, fecgpu_rlc_decode_apply_packed
 * and a scatter under recovered[].  The length tables are device-accessible arrays: the kernels clamp
 * them as above instead of checking (fecgpu_rlc_decode_rows_len_host checks before any launch). */
int fecgpu_rlc_decode_rows_len(const uint64_t *src_rows, const uint32_t *src_len, const uint64_t *rep_rows,
                               const uint32_t *rep_len, const uint32_t *blk_len, uint64_t nblocks, uint32_t k,
                               uint32_t r, uint32_t symbol_size, const uint32_t *rep_seed,
                               const uint64_t *src_present, const uint64_t *rep_present, uint8_t *status,
                               uint64_t *recovered, void *workspace, size_t workspace_bytes, void *stream);

/* The same on ragged rows in ONE pass over memory: no gather, no packed batch, no scatter.  The data
 * kernels of fecgpu_rlc_encode_rows / fecgpu_rlc_decode_rows run length-aware bodies that read every
 * input row through a buffer descriptor bounded by its own length (bytes past it count as zero and are
 * not read) and store exactly blk_len[b] bytes per output row.  Tables, lengths, clamping (blk_len to
 * symbol_size, src_len / rep_len to blk_len[b]) and address rules are those of the *_rows_len forms: rows
 * 4-byte aligned, below 2^48, in device memory or mapped page-locked host memory; a row of 0 bytes and
 * an absent row are never dereferenced and may have address 0; a load may touch the aligned dword that
 * holds a row's last byte and nothing after it; stores are 16-B / dword stores and byte stores for the
 * last 1-3 bytes, no dword is read-modify-written, nothing is written past blk_len[b] bytes of a row.
 * Encode needs no workspace and writes to every repair row the bytes fecgpu_rlc_encode_rows_len writes.
 * Decode needs fecgpu_rlc_decode_workspace(nblocks, k, r) only; status[] and recovered[] are exactly what
 * fecgpu_rlc_decode_seeded gives on the zero-padded rows, and every missing source whose recovered bit is
 * set holds its blk_len[b] bytes.  As in fecgpu_rlc_decode_rows the data pass writes the unknown rows of a
 * RECOVERED block before the zero/undetermined rule is known, so -- unlike fecgpu_rlc_decode_rows_len -- a
 * missing source of a RECOVERED block whose bit stays clear may have received blk_len[b] bytes too (the
 * reference's unspecified bytes).  Blocks of any other status are neither read nor written.  Both calls
 * are asynchronous on `stream`, allocate nothing and can be captured into a graph. */
int fecgpu_rlc_encode_rows_fused(const uint64_t *src_rows, const uint32_t *src_len, const uint64_t *rep_rows,
                                 const uint32_t *blk_len, uint64_t nblocks, uint32_t k, uint32_t r,
                                 uint32_t symbol_size, uint32_t fbn_base, const uint32_t *fbn, void *stream);
int fecgpu_rlc_decode_rows_fused(const uint64_t *src_rows, const uint32_t *src_len, const uint64_t *rep_rows,
                                 const uint32_t *rep_len, const uint32_t *blk_len, uint64_t nblocks, uint32_t k,
                                 uint32_t r, uint32_t symbol_size, const uint32_t *rep_seed,
                                 const uint64_t *src_present, const uint64_t *rep_present, uint8_t *status,
                                 uint64_t *recovered, void *workspace, size_t workspace_bytes, void *stream);
/* fecgpu_rlc_decode_rows_fused in full-rank mode: status[] and recovered[] are what fecgpu_rlc_decode_full
 * with rep_seed gives on the zero-padded rows; lengths, clamping and address rules as above.  A repair
 * full mode does not select is never dereferenced; a SINGULAR block reads and writes no row.  (The
 * *_rows_len forms have no full-rank counterpart.) */
int fecgpu_rlc_decode_rows_fused_full(const uint64_t *src_rows, const uint32_t *src_len, const uint64_t *rep_rows,
                                      const uint32_t *rep_len, const uint32_t *blk_len, uint64_t nblocks, uint32_t k,
                                      uint32_t r, uint32_t symbol_size, const uint32_t *rep_seed,
                                      const uint64_t *src_present, const uint64_t *rep_present, uint8_t *status,
                                      uint64_t *recovered, void *workspace, size_t workspace_bytes, void *stream);

/* XOR encode (r == 1): rep[b][0] = XOR_j src[b][j]. */
int fecgpu_xor_encode(const void *src, void *rep, uint64_t nblocks, uint32_t k,
                      uint32_t symbol_size, void *stream);

/* XOR on rows given by address, each of its own length, in one pass: no packed intermediate and no
 * workspace.  src_rows[b * k + j] / src_len[b * k + j] are the address and length of source j of block b,
 * rep_rows[b] ([nblocks]) the address of its one repair row and blk_len[b] the block's length (the
 * reference's max_length).  The kernels clamp blk_len to symbol_size and src_len to blk_len, as the RLC
 * *_rows_len forms do (the host forms check both before any launch).
 * Encode writes exactly blk_len[b] bytes to the repair row: byte t is the XOR over j of source j's byte t,
 * taken as 0 for t >= src_len (xor_fec_scheme_generate.c:51-73).
 * Decode computes status[] and recovered[] exactly as fecgpu_xor_decode does from the masks clipped to k:
 * RECOVERED iff popcount(sources present) + repair present == k and the repair is present, REF_UB when the
 * sum holds with the repair absent, NOTHING otherwise; the bit of the missing index is set (also when the
 * recovered bytes are all zero).  For a RECOVERED block exactly blk_len[b] bytes go to the missing source's
 * own row, src_rows[b * k + miss]: the repair (read for blk_len[b] bytes) ^ the present sources, each read
 * for min(src_len, blk_len[b]) bytes -- a received source longer than the block is truncated
 * (xor_fec_scheme.c:54-70).  For any other status no row is read or written.
 * Memory rules, those of the ragged copy kernels above: row addresses are 4-byte aligned, in device memory
 * or mapped page-locked host memory; a row of 0 bytes is never dereferenced and its address may be 0, and
 * so may that of an absent source or an absent repair; a load may touch the aligned dword that holds a
 * row's last byte and nothing after it; stores are 16-B, then dword, then byte stores for the last 1-3
 * bytes -- no dword is read-modify-written and nothing is written past blk_len[b].  The tables are
 * device-accessible arrays.  k is 1..128, symbol_size a multiple of 4 from 4 to 65532.  Callers with packed
 * rows keep fecgpu_xor_encode / fecgpu_xor_decode. */
int fecgpu_xor_encode_rows(const uint64_t *src_rows, const uint32_t *src_len, const uint64_t *rep_rows,
                           const uint32_t *blk_len, uint64_t nblocks, uint32_t k, uint32_t symbol_size, void *stream);
int fecgpu_xor_decode_rows(const uint64_t *src_rows, const uint32_t *src_len, const uint64_t *rep_rows,
                           const uint32_t *blk_len, uint64_t nblocks, uint32_t k, uint32_t symbol_size,
                           const uint64_t *src_present, const uint64_t *rep_present, uint8_t *status,
                           uint64_t *recovered, void *stream);

/* RLC decode.  Presence masks: bit j of src_present[2*b + j/64] set <=> source j of
 * block b was received; same for rep_present.  Recovered sources are written IN PLACE
 * into src[b][j]; bit j of recovered[2*b + j/64] is set for every source the reference
 * would insert (determined and non-zero, rlc_fec_scheme_gf256.c:218-236).  Bytes of a
 * missing slot whose bit stays clear are unspecified.  `workspace` must hold
 * fecgpu_rlc_decode_workspace(nblocks, k, r) bytes of device memory. */
size_t fecgpu_rlc_decode_workspace(uint64_t nblocks, uint32_t k, uint32_t r);
int fecgpu_rlc_decode(void *src, const void *rep, uint64_t nblocks, uint32_t k, uint32_t r,
                      uint32_t symbol_size, uint32_t fbn_base, const uint32_t *fbn,
                      const uint64_t *src_present, const uint64_t *rep_present,
                      uint8_t *status, uint64_t *recovered, void *workspace,
                      size_t workspace_bytes, void *stream);

/* The two stages fecgpu_rlc_decode runs, for callers that schedule or time them apart:
 * plan  -- coefficient-only replay of the reference elimination per block (workspace);
 * apply -- the data pass (e recovered symbols from k received ones, written in place) and the
 *          reference's zero/undetermined rule, writing status[] and recovered[].  When
 *          min(k, r) <= 16 the rule runs inside the data kernel; otherwise apply launches one
 *          more small kernel after the data passes. */
int fecgpu_rlc_decode_plan(uint64_t nblocks, uint32_t k, uint32_t r, uint32_t fbn_base,
                           const uint32_t *fbn, const uint64_t *src_present,
                           const uint64_t *rep_present, void *workspace, size_t workspace_bytes,
                           void *stream);
int fecgpu_rlc_decode_apply(void *src, const void *rep, uint64_t nblocks, uint32_t k, uint32_t r,
                            uint32_t symbol_size, uint8_t *status, uint64_t *recovered,
                            void *workspace, size_t workspace_bytes, void *stream);
/* apply with the recovered symbols written to dst instead of in place: dst has src's layout
 * ([block][k][symbol_size]) and receives only the recovered rows (every other byte of dst is left
 * untouched); src is only read.  dst may be any memory the device can write -- e.g. page-locked
 * host packet buffers, so recovered symbols cross PCIe once and nothing else comes back
 * (fecgpu_rlc_decode_host uses this for pinned buffers). */
int fecgpu_rlc_decode_apply_to(const void *src, const void *rep, void *dst, uint64_t nblocks,
                               uint32_t k, uint32_t r, uint32_t symbol_size, uint8_t *status,
                               uint64_t *recovered, void *workspace, size_t workspace_bytes,
                               void *stream);
/* apply with the recovered symbols packed: dst is [nblocks][min(k, r)][symbol_size] and row u of
 * block b receives the u-th missing source of b in ascending source order (the u-th clear bit of
 * src_present below k); rows past the block's erasures and rows whose recovered[] bit stays clear are
 * unspecified.  The reference's fec_recover allocates every recovered symbol anew
 * (rlc_fec_scheme_gf256.c:218-236), so a packed row per recovered symbol is as faithful as src's
 * layout, and a block's rows are contiguous: no written row shares a cache line with bytes the pass
 * does not write (recovered rows at their src-layout slots leave two half-written 128-B lines each,
 * which the memory system fetches to merge). */
int fecgpu_rlc_decode_apply_packed(const void *src, const void *rep, void *dst, uint64_t nblocks,
                                   uint32_t k, uint32_t r, uint32_t symbol_size, uint8_t *status,
                                   uint64_t *recovered, void *workspace, size_t workspace_bytes,
                                   void *stream);

/* RLC decode with the coefficients of every received repair seeded by its own FPID, as the
 * reference does (get_coefs(..., rs->repair_fec_payload_id.source_fpid.raw, ...),
 * rlc_fec_scheme_gf256.c:200): rep_seed[b * r + i] is the low 32 bits of the FPID of the repair
 * in slot i of block b (entries of absent repairs are ignored).  This is the general form: the
 * block framework's repairs carry (fbn << 8) | i, which is what fecgpu_rlc_decode assumes, but
 * the sliding-window framework's blocks are numbered by their window start while their repairs
 * carry block number 0 (window_framework_receiver.h:60-86, window_framework_sender.h:239-243).
 * Recovered FPIDs are the caller's business (the host adapters stamp (fec_block_number << 8) + j,
 * :222). */
int fecgpu_rlc_decode_plan_seeded(uint64_t nblocks, uint32_t k, uint32_t r, const uint32_t *rep_seed,
                                  const uint64_t *src_present, const uint64_t *rep_present, void *workspace,
                                  size_t workspace_bytes, void *stream);
int fecgpu_rlc_decode_seeded(void *src, const void *rep, uint64_t nblocks, uint32_t k, uint32_t r,
                             uint32_t symbol_size, const uint32_t *rep_seed, const uint64_t *src_present,
                             const uint64_t *rep_present, uint8_t *status, uint64_t *recovered, void *workspace,
                             size_t workspace_bytes, void *stream);

/* Full-rank RLC decode (opt-in; fecgpu_rlc_decode and its kin stay reference-faithful, bit for bit).
 * The reference's elimination uses the first n = k - received sources repairs, sorts the rows once,
 * never re-pivots and walks off its array on a zero pivot (FECGPU_BLOCK_REF_UB) -- on 1-5 % of random
 * erasure patterns, almost all of which the received symbols determine.  Full mode recovers every block
 * they determine.  Per block, with the masks clipped to k and r and m = received repairs:
 *   FECGPU_BLOCK_NOTHING    the same preconditions as fecgpu_rlc_decode (r == 0, no source missing, or
 *                           received sources + m < k);
 *   FECGPU_BLOCK_RECOVERED  the m x n matrix of the received repairs' TinyMT32 rows, restricted to the
 *                           missing columns, has rank n: every missing source is solved and written.  The
 *                           solution is unique, so the bytes are the original sources (and
 *                           fecgpu_rlc_decode's bytes wherever that recovers).  Exactly n received repairs
 *                           are used, the lowest-index independent set; absent and unused repairs are
 *                           never read.  recovered[] has the bit of every missing source whose bytes are
 *                           not all zero; an all-zero one is written as zeros with its bit clear (as in
 *                           reference mode), but it never hides another symbol;
 *   FECGPU_BLOCK_SINGULAR   rank < n: nothing is written for the block, recovered[] is 0.
 * FECGPU_BLOCK_REF_UB is never returned.  rep_seed selects the seeding: non-NULL, every equation is seeded
 * by rep_seed[b * r + i] as in fecgpu_rlc_decode_seeded (fbn_base and fbn are ignored); NULL, by
 * (fbn_b << 8) | i as in fecgpu_rlc_decode.  Workspace, masks, status and recovered as fecgpu_rlc_decode.
 * fecgpu_rlc_decode_plan_full writes the same plan records as fecgpu_rlc_decode_plan (the reference plan,
 * then a fix-up pass that re-plans the blocks it gave up on) and pairs with fecgpu_rlc_decode_apply,
 * _apply_to and _apply_packed; fecgpu_rlc_decode_full is plan_full + apply as separate launches, except that
 * a batch of up to 64 blocks with at most 16 unknowns each whose rows fit a workgroup's LDS is one launch (the
 * one-block kernel re-plans a given-up block in place); knob plan != 0 forces the separate launches.  The
 * outputs are the same either way. */
int fecgpu_rlc_decode_plan_full(uint64_t nblocks, uint32_t k, uint32_t r, uint32_t fbn_base, const uint32_t *fbn,
                                const uint32_t *rep_seed, const uint64_t *src_present, const uint64_t *rep_present,
                                void *workspace, size_t workspace_bytes, void *stream);
int fecgpu_rlc_decode_full(void *src, const void *rep, uint64_t nblocks, uint32_t k, uint32_t r,
                           uint32_t symbol_size, uint32_t fbn_base, const uint32_t *fbn, const uint32_t *rep_seed,
                           const uint64_t *src_present, const uint64_t *rep_present, uint8_t *status,
                           uint64_t *recovered, void *workspace, size_t workspace_bytes, void *stream);

/* Span decode (opt-in): the joint decode of the sliding-window framework's overlapping windows.  Every
 * other decode treats a window as a closed block, so a repair helps only the window it was sent with,
 * although a source symbol lies in k / step windows.  A span is K consecutive stream symbols (1..128) and
 * R repair slots (1..128) for the received repairs whose windows lie inside it, with presence masks as
 * everywhere else.  Repair slot i of span b carries rep_seed[b * R + i] (its FPID, as in
 * fecgpu_rlc_decode_seeded), rep_off[b * R + i] (the first column its window covers) and
 * rep_nss[b * R + i] (its window's length): its coefficient row is zero outside [off, off + nss) and the
 * first nss TinyMT32 coefficients of the seed inside, what the sender used for that window.  A present
 * repair with nss == 0 or off + nss > K counts as absent.
 * With n missing columns, m present valid repairs and M their m x n matrix on the missing columns, missing
 * column u is determined iff e_u lies in the row space of M.  Per span:
 *   FECGPU_BLOCK_NOTHING    n == 0 or m == 0;
 *   FECGPU_BLOCK_RECOVERED  at least one column is determined: every determined source is written (the
 *                           bytes are unique, so they are the original symbol), no other row is.
 *                           recovered[] has the bit of every determined source whose bytes are not all
 *                           zero; an all-zero one is written with its bit clear, as in full-rank mode;
 *   FECGPU_BLOCK_SINGULAR   none is determined: no row is read or written.
 * FECGPU_BLOCK_REF_UB is never returned, and the reference's received + m >= k precondition does not
 * apply: fewer repairs than losses can still determine some of them.  Only the lowest-index independent
 * set of repairs is read (the greedy scan in ascending slot order); a repair that is absent, invalid,
 * dependent on earlier ones or zero on every missing column is never dereferenced.  Where every repair has
 * off == 0 and nss == K, and fecgpu_rlc_decode_full with rep_seed recovers the span (or has n == 0 or
 * m == 0), status, recovered[] and bytes are identical to it.
 * The workspace is fecgpu_rlc_decode_workspace(nspans, K, R); fecgpu_rlc_span_decode_plan writes the plan
 * records every decode shares and pairs with fecgpu_rlc_decode_apply, _apply_to and _apply_packed (packed
 * row u = the u-th determined source, ascending); fecgpu_rlc_span_decode is the plan and the in-place apply
 * on packed rows src[span][K][L], rep[span][R][L].  Argument errors (K or R out of range, NULL tables,
 * misalignment, a workspace that is too small) return FECGPU_ERR_INVALID before anything is launched.
 * Asynchronous on `stream`, nothing allocated.
 * Knob "span_compact" (fecgpu_set_knob; 0/1, default 1): the data pass of a span decode -- these entry
 * points, the row forms below, and an apply call on the workspace the last fecgpu_rlc_span_decode_plan call
 * filled -- lists per tile of unknowns only the input rows with a non-zero coefficient for one of them, so a
 * row no unknown of the tile depends on is not read; 0 streams all K columns as before.  Same bytes either
 * way.  The LDS-ring tiles (16 unknowns on packed rows, knob "ring") keep all K; the reference-faithful and
 * full-rank decodes never compact. */
int fecgpu_rlc_span_decode_plan(uint64_t nspans, uint32_t K, uint32_t R, const uint32_t *rep_seed,
                                const uint8_t *rep_off, const uint8_t *rep_nss, const uint64_t *src_present,
                                const uint64_t *rep_present, void *workspace, size_t workspace_bytes, void *stream);
int fecgpu_rlc_span_decode(void *src, const void *rep, uint64_t nspans, uint32_t K, uint32_t R, uint32_t symbol_size,
                           const uint32_t *rep_seed, const uint8_t *rep_off, const uint8_t *rep_nss,
                           const uint64_t *src_present, const uint64_t *rep_present, uint8_t *status,
                           uint64_t *recovered, void *workspace, size_t workspace_bytes, void *stream);
/* The span decode on rows by address with a length each: the tables, lengths, clamping and address rules
 * of fecgpu_rlc_decode_rows_fused_full, plus rep_off and rep_nss.  blk_len[b] is the span's length; a
 * repair shorter than it counts as zero-padded, which is exact (every source of that window is at most as
 * long).  Every determined source receives exactly blk_len[b] bytes at its own row; no other row is
 * written, nothing is written past blk_len[b], and a repair the plan does not select is never
 * dereferenced.
 * One launch for a few spans: with nspans <= 64, knob "plan" at 0 (as for fecgpu_rlc_decode_full: knob plan
 * != 0 forces the separate launches) and a shape whose plan scratch and plan record fit 64 KiB of LDS
 * together (K 128 with R 32 does, about 21 KiB; K = R = 128 does not), one kernel plans each span and runs
 * its data pass in tiles of at most 8 unknowns, the record never leaving LDS.  Arguments, checks, outputs
 * and the workspace requirement are the same; the workspace is not written on that path.  Every other call
 * runs the plan kernel, a data-pass launch per tile of unknowns and the finalize kernel.  Same bytes either
 * way.  fecgpu_rlc_span_decode and the plan / apply pair always keep their launches. */
int fecgpu_rlc_span_decode_rows_fused(const uint64_t *src_rows, const uint32_t *src_len, const uint64_t *rep_rows,
                                      const uint32_t *rep_len, const uint32_t *blk_len, uint64_t nspans, uint32_t K,
                                      uint32_t R, uint32_t symbol_size, const uint32_t *rep_seed,
                                      const uint8_t *rep_off, const uint8_t *rep_nss, const uint64_t *src_present,
                                      const uint64_t *rep_present, uint8_t *status, uint64_t *recovered,
                                      void *workspace, size_t workspace_bytes, void *stream);
/* The fecgpu_rlc_span_decode_rows_fused calls of this process that ran as one launch (the rule above). */
uint64_t fecgpu_rlc_span_one_launch_calls(void);
/* From a receiver's window to a span (host only, no device): first_id[i] and nss[i] are the window start
 * (the repair's fec_scheme_specific) and length of received repair i, m of them.  Differences are taken
 * modulo 2^32 from first_id[0], so ids may wrap.  *base_id is the span's first symbol id, *K its width,
 * off[i] repair i's first column.  FECGPU_ERR_INVALID when m == 0, a pointer is NULL or the width
 * exceeds 128. */
int fecgpu_rlc_span_layout(const uint32_t *first_id, const uint8_t *nss, uint32_t m, uint32_t *base_id, uint32_t *K,
                           uint8_t *off);

/* XOR decode (r == 1), same conventions. */
int fecgpu_xor_decode(void *src, const void *rep, uint64_t nblocks, uint32_t k,
                      uint32_t symbol_size, const uint64_t *src_present,
                      const uint64_t *rep_present, uint8_t *status, uint64_t *recovered,
                      void *stream);
/* fecgpu_xor_decode with the recovered symbol of block b written to dst + b * symbol_size (one row per
 * block, as fec_recover allocates the recovered symbol anew, xor_fec_scheme.c:54-58) instead of into
 * src; src is not written.  Rows of blocks with nothing recovered are left as they were. */
int fecgpu_xor_decode_to(const void *src, const void *rep, void *dst, uint64_t nblocks, uint32_t k,
                         uint32_t symbol_size, const uint64_t *src_present,
                         const uint64_t *rep_present, uint8_t *status, uint64_t *recovered,
                         void *stream);

/* ---- Host-resident path --------------------------------------------------------------------
 * The same operations on HOST buffers (pageable or pinned): H2D copy, kernels, D2H copy,
 * pipelined over sub-batches of about `chunk_bytes` of payload on `nstreams` HIP streams so
 * that PCIe transfers overlap the kernels.  Synchronous: results are in host memory on
 * return.  Used by the protoop adapters (one block per call) and by the PCIe-inclusive
 * measurement.  Page-locked buffers (fecgpu_host_alloc, hipHostMalloc, registered) are zero-copy:
 * the kernels read the blocks and write repairs / recovered rows directly over PCIe, so only the
 * bytes the operation needs cross the bus.  Pageable buffers are staged by copies (decode then
 * copies whole source rows back). */
typedef struct fecgpu_host_ctx fecgpu_host_ctx_t;
fecgpu_host_ctx_t *fecgpu_host_ctx_create(int device, int nstreams, size_t chunk_bytes);
void fecgpu_host_ctx_destroy(fecgpu_host_ctx_t *ctx);
int fecgpu_rlc_encode_host(fecgpu_host_ctx_t *ctx, const void *src, void *rep, uint64_t nblocks,
                           uint32_t k, uint32_t r, uint32_t symbol_size, uint32_t fbn_base,
                           const uint32_t *fbn);
int fecgpu_rlc_decode_host(fecgpu_host_ctx_t *ctx, void *src, const void *rep, uint64_t nblocks,
                           uint32_t k, uint32_t r, uint32_t symbol_size, uint32_t fbn_base,
                           const uint32_t *fbn, const uint64_t *src_present,
                           const uint64_t *rep_present, uint8_t *status, uint64_t *recovered);
/* host-resident fecgpu_rlc_decode_seeded: rep_seed is a host array [nblocks][r] */
int fecgpu_rlc_decode_host_seeded(fecgpu_host_ctx_t *ctx, void *src, const void *rep, uint64_t nblocks,
                                  uint32_t k, uint32_t r, uint32_t symbol_size, const uint32_t *rep_seed,
                                  const uint64_t *src_present, const uint64_t *rep_present, uint8_t *status,
                                  uint64_t *recovered);
/* host-resident fecgpu_rlc_decode_full: fbn / rep_seed are host arrays ([nblocks] / [nblocks][r]) */
int fecgpu_rlc_decode_host_full(fecgpu_host_ctx_t *ctx, void *src, const void *rep, uint64_t nblocks,
                                uint32_t k, uint32_t r, uint32_t symbol_size, uint32_t fbn_base,
                                const uint32_t *fbn, const uint32_t *rep_seed, const uint64_t *src_present,
                                const uint64_t *rep_present, uint8_t *status, uint64_t *recovered);
/* fecgpu_rlc_encode_rows from the host: the row tables and fbn[] are host arrays (page-locked arrays
 * are read in place, others are copied), the rows themselves must be device-accessible. */
int fecgpu_rlc_encode_rows_host(fecgpu_host_ctx_t *ctx, const uint64_t *src_rows, const uint64_t *rep_rows,
                                uint64_t nblocks, uint32_t k, uint32_t r, uint32_t symbol_size, const uint32_t *fbn);
/* fecgpu_rlc_decode_rows from the host: the row tables, seeds, masks, status and recovered are host
 * arrays (page-locked ones are used in place, others copied); the rows must be device-accessible.  With
 * r == 0 the repair table and the seeds have no entries and are not read (NULL is accepted). */
int fecgpu_rlc_decode_rows_host(fecgpu_host_ctx_t *ctx, const uint64_t *src_rows, const uint64_t *rep_rows,
                                uint64_t nblocks, uint32_t k, uint32_t r, uint32_t symbol_size,
                                const uint32_t *rep_seed, const uint64_t *src_present, const uint64_t *rep_present,
                                uint8_t *status, uint64_t *recovered);
/* the same in full-rank mode (fecgpu_rlc_decode_rows_full): same staging, same slices */
int fecgpu_rlc_decode_rows_host_full(fecgpu_host_ctx_t *ctx, const uint64_t *src_rows, const uint64_t *rep_rows,
                                     uint64_t nblocks, uint32_t k, uint32_t r, uint32_t symbol_size,
                                     const uint32_t *rep_seed, const uint64_t *src_present,
                                     const uint64_t *rep_present, uint8_t *status, uint64_t *recovered);
/* fecgpu_rlc_encode_rows_len / fecgpu_rlc_decode_rows_len from the host: the row tables, length tables,
 * fbn[] / seeds, masks, status and recovered are host arrays (page-locked ones are used in place,
 * others are copied); the rows must be device-accessible.  The batch runs in sub-batches of about
 * chunk_bytes of payload whose packed arrays live in the context's own device buffers.  Before any
 * launch both check blk_len[b] <= symbol_size and src_len <= blk_len[b] (decode: for the sources
 * present) and return FECGPU_ERR_INVALID otherwise, with nothing written.  With r == 0 decode does not
 * read the repair tables and seeds (NULL is accepted). */
int fecgpu_rlc_encode_rows_len_host(fecgpu_host_ctx_t *ctx, const uint64_t *src_rows, const uint32_t *src_len,
                                    const uint64_t *rep_rows, const uint32_t *blk_len, uint64_t nblocks, uint32_t k,
                                    uint32_t r, uint32_t symbol_size, const uint32_t *fbn);
int fecgpu_rlc_decode_rows_len_host(fecgpu_host_ctx_t *ctx, const uint64_t *src_rows, const uint32_t *src_len,
                                    const uint64_t *rep_rows, const uint32_t *rep_len, const uint32_t *blk_len,
                                    uint64_t nblocks, uint32_t k, uint32_t r, uint32_t symbol_size,
                                    const uint32_t *rep_seed, const uint64_t *src_present,
                                    const uint64_t *rep_present, uint8_t *status, uint64_t *recovered);
/* fecgpu_rlc_encode_rows_fused / fecgpu_rlc_decode_rows_fused from the host: arguments, staging of the host
 * arrays and the checks before any launch are those of the *_rows_len_host forms; the sub-batches need
 * none of the context's packed device buffers (decode uses its plan workspace only). */
int fecgpu_rlc_encode_rows_fused_host(fecgpu_host_ctx_t *ctx, const uint64_t *src_rows, const uint32_t *src_len,
                                      const uint64_t *rep_rows, const uint32_t *blk_len, uint64_t nblocks,
                                      uint32_t k, uint32_t r, uint32_t symbol_size, const uint32_t *fbn);
int fecgpu_rlc_decode_rows_fused_host(fecgpu_host_ctx_t *ctx, const uint64_t *src_rows, const uint32_t *src_len,
                                      const uint64_t *rep_rows, const uint32_t *rep_len, const uint32_t *blk_len,
                                      uint64_t nblocks, uint32_t k, uint32_t r, uint32_t symbol_size,
                                      const uint32_t *rep_seed, const uint64_t *src_present,
                                      const uint64_t *rep_present, uint8_t *status, uint64_t *recovered);
/* fecgpu_rlc_decode_rows_fused_host in full-rank mode (fecgpu_rlc_decode_rows_fused_full) */
int fecgpu_rlc_decode_rows_fused_host_full(fecgpu_host_ctx_t *ctx, const uint64_t *src_rows, const uint32_t *src_len,
                                           const uint64_t *rep_rows, const uint32_t *rep_len, const uint32_t *blk_len,
                                           uint64_t nblocks, uint32_t k, uint32_t r, uint32_t symbol_size,
                                           const uint32_t *rep_seed, const uint64_t *src_present,
                                           const uint64_t *rep_present, uint8_t *status, uint64_t *recovered);
/* fecgpu_rlc_span_decode_rows_fused from the host: host tables, staged like those of the other table forms.
 * Before any launch it checks blk_len and the lengths as fecgpu_rlc_decode_rows_fused_host does, and
 * rep_off + rep_nss <= K for every present repair (FECGPU_ERR_INVALID). */
int fecgpu_rlc_span_decode_rows_fused_host(fecgpu_host_ctx_t *ctx, const uint64_t *src_rows, const uint32_t *src_len,
                                           const uint64_t *rep_rows, const uint32_t *rep_len, const uint32_t *blk_len,
                                           uint64_t nspans, uint32_t K, uint32_t R, uint32_t symbol_size,
                                           const uint32_t *rep_seed, const uint8_t *rep_off, const uint8_t *rep_nss,
                                           const uint64_t *src_present, const uint64_t *rep_present, uint8_t *status,
                                           uint64_t *recovered);
/* fecgpu_rlc_window_encode_table from the host: the stream (host rows) crosses PCIe once, by one copy,
 * before the windows are coded from device memory -- a symbol serves up to k windows, so reading it in
 * place would cross the bus that many times; wrow[] is a host array; repairs go to page-locked `rep` in
 * place, others by a copy.  With knob window_sc 0 the windows run through the row-table kernel. */
int fecgpu_rlc_window_encode_host(fecgpu_host_ctx_t *ctx, const void *symbols, uint64_t nrows, const uint32_t *wrow,
                                  uint64_t nwindows, uint32_t k, uint32_t r, uint32_t symbol_size, void *rep);
/* fecgpu_rlc_window_encode_rows from the host: the five tables are host arrays (all used in place when
 * all are page-locked, otherwise all copied once into one device buffer); the rows must be
 * device-accessible.  The context grows its own stream workspace; the call runs unsliced, one stream
 * serving all its windows.  Before the context is looked at it checks the shapes, NULL tables,
 * wrow[w] + k <= nrows, row_len[x] <= symbol_size and blk_len[w] <= symbol_size, and returns
 * FECGPU_ERR_INVALID with a message naming the rule, nothing written.  With knob window_sc 0, or a stream
 * past the kernel's 32-bit offsets, the windows are expanded to blocks (src_rows[w * k + j] =
 * rows[wrow[w] + j]) and run through fecgpu_rlc_encode_rows_fused_host with every block number 0: the same
 * bytes, each symbol read once per window. */
int fecgpu_rlc_window_encode_rows_host(fecgpu_host_ctx_t *ctx, const uint64_t *rows, const uint32_t *row_len,
                                       uint64_t nrows, const uint32_t *wrow, const uint64_t *rep_rows,
                                       const uint32_t *blk_len, uint64_t nwindows, uint32_t k, uint32_t r,
                                       uint32_t symbol_size);
/* fecgpu_rlc_window_encode_rows_host for windows of their own length (the window sender protects whatever is
 * in flight, 1 to 30 symbols, window_framework_sender.h:209-260): window w protects rows wrow[w] ..
 * wrow[w] + wlen[w] - 1 with block number 0, wlen[w] in 1..kmax.  Repair row (w, i) receives exactly
 * blk_len[w] bytes, those of an RLC encode of block 0 over these rows and r repairs, every row counting for
 * min(row_len, blk_len[w]) bytes.  The coefficient of (position j, repair i) does not depend on the
 * window's length, so the call sorts the windows into classes of one length
 * (fecgpu_rlc_window_classes) and one launch per tile of 8 repairs codes them all, a 2 KiB chunk never
 * holding two lengths.  Memory rules, alignment rules, clamps and the staging of the tables (perm and the
 * class table go with them: in place when page-locked, else copied once) are those of
 * fecgpu_rlc_window_encode_rows_host.  Before the context is looked at it checks NULL tables, the ranges
 * of kmax, r and symbol_size, wlen[w] in 1..kmax ("wlen"), wrow[w] + wlen[w] <= nrows ("wrow"),
 * row_len[x] <= symbol_size and blk_len[w] <= symbol_size, and returns FECGPU_ERR_INVALID with a message
 * naming the rule, nothing written.  nwindows == 0 is FECGPU_OK without a launch.  When every wlen[w]
 * equals kmax the call is fecgpu_rlc_window_encode_rows_host itself.  With knob window_sc 0, or
 * (nrows + kmax) * width at 2 GiB or more, every window becomes a block of kmax rows through
 * fecgpu_rlc_encode_rows_fused_host with block number 0, the positions past wlen[w] given as rows of
 * length 0 and address 0 (never dereferenced): the same bytes. */
int fecgpu_rlc_window_encode_rows_var_host(fecgpu_host_ctx_t *ctx, const uint64_t *rows, const uint32_t *row_len,
                                           uint64_t nrows, const uint32_t *wrow, const uint8_t *wlen,
                                           const uint64_t *rep_rows, const uint32_t *blk_len, uint64_t nwindows,
                                           uint32_t kmax, uint32_t r, uint32_t symbol_size);
/* The sort behind it (host only, no device): a stable counting sort of the windows by length.  perm[p] is
 * the window at sorted position p (within a class the windows keep the caller's order, so neighbouring
 * windows of one connection stay neighbours in time); the classes follow in order of length, class x
 * holding cnt[x] windows of len[x] symbols from sorted position first[x], its windows x bytes space
 * (cnt[x] * width, the width being symbol_size rounded up to 16) cut into 2 KiB chunks of its own from
 * chunk cchunk[x] on.  cls holds four arrays of kmax entries, first[], cnt[], len[], cchunk[], in that
 * order; entries past *nclasses are 0, their cchunk 2^32 - 1.  *nchunks = sum of ceil(cnt[x] * width /
 * 2048).  FECGPU_ERR_INVALID, with a message naming the rule, for a NULL pointer, kmax outside 1..128, a
 * symbol_size the encode would refuse, any wlen[w] outside 1..kmax, or 2^32 - 1 windows or chunks. */
int fecgpu_rlc_window_classes(const uint8_t *wlen, uint64_t nwin, uint32_t kmax, uint32_t symbol_size,
                              uint32_t *perm, uint32_t *cls /* [4 * kmax]: first, cnt, len, first chunk */,
                              uint32_t *nclasses, uint64_t *nchunks);
int fecgpu_xor_encode_host(fecgpu_host_ctx_t *ctx, const void *src, void *rep, uint64_t nblocks,
                           uint32_t k, uint32_t symbol_size);
int fecgpu_xor_decode_host(fecgpu_host_ctx_t *ctx, void *src, const void *rep, uint64_t nblocks,
                           uint32_t k, uint32_t symbol_size, const uint64_t *src_present,
                           const uint64_t *rep_present, uint8_t *status, uint64_t *recovered);
/* fecgpu_xor_encode_rows / fecgpu_xor_decode_rows from the host: the tables, masks, status and recovered
 * are host arrays (page-locked ones are used in place, others are copied); the rows must be
 * device-accessible.  The batch runs in sub-batches of about chunk_bytes of payload over the context's
 * streams.  Before the context is looked at both check blk_len[b] <= symbol_size and src_len <= blk_len[b]
 * (decode: for the sources present) and return FECGPU_ERR_INVALID otherwise, with nothing written.  Packed
 * host rows keep fecgpu_xor_encode_host / fecgpu_xor_decode_host. */
int fecgpu_xor_encode_rows_host(fecgpu_host_ctx_t *ctx, const uint64_t *src_rows, const uint32_t *src_len,
                                const uint64_t *rep_rows, const uint32_t *blk_len, uint64_t nblocks, uint32_t k,
                                uint32_t symbol_size);
int fecgpu_xor_decode_rows_host(fecgpu_host_ctx_t *ctx, const uint64_t *src_rows, const uint32_t *src_len,
                                const uint64_t *rep_rows, const uint32_t *blk_len, uint64_t nblocks, uint32_t k,
                                uint32_t symbol_size, const uint64_t *src_present, const uint64_t *rep_present,
                                uint8_t *status, uint64_t *recovered);

/* ---- Resident single-block service (the synchronous hooks) ------------------------------------
 * One block per call, as the block framework calls fec_generate_repair_symbols / fec_recover
 * (block_framework_sender.h:187, fec_protoops.h:246): a worker workgroup stays resident on the device
 * and polls a page-locked mailbox, so a call costs a mailbox round trip over PCIe instead of a
 * kernel launch.  The worker ends by itself after 20 ms without a request (and after 50 ms in all);
 * the next call relaunches it.  It runs on a stream of the greatest priority (its own hardware queue
 * unless the process creates other such streams), so the process's other kernels do not queue behind it.  Every buffer must be page-locked (fecgpu_host_alloc, registered
 * ranges); the rows are zero-copy.  Returns FECGPU_ERR_INVALID when the block does not fit the
 * worker (e > 16 unknowns, rows beyond its LDS), a buffer is not page-locked, knob block_svc is 0, or
 * the request was withdrawn at its deadline (below) -- the caller then takes the host path.
 * Thread-safe (one request at a time per service). */
typedef struct fecgpu_block_svc fecgpu_block_svc_t;
fecgpu_block_svc_t *fecgpu_block_svc_create(int device);
void fecgpu_block_svc_destroy(fecgpu_block_svc_t *svc);
/* rep[i] = sum_j coef((fbn << 8) | i)[j] * src[j] for one block (k rows of symbol_size bytes) */
int fecgpu_block_svc_rlc_encode(fecgpu_block_svc_t *svc, const void *src, void *rep, uint32_t k, uint32_t r,
                                uint32_t symbol_size, uint32_t fbn);
/* fecgpu_rlc_decode_seeded for one block; recovered rows go to dst (src's layout), src is only read */
int fecgpu_block_svc_rlc_decode_seeded(fecgpu_block_svc_t *svc, const void *src, const void *rep, void *dst,
                                       uint32_t k, uint32_t r, uint32_t symbol_size, const uint32_t *rep_seed,
                                       const uint64_t *src_present, const uint64_t *rep_present, uint8_t *status,
                                       uint64_t *recovered);
/* The same in full-rank mode (fecgpu_rlc_decode_full with rep_seed, one block): the worker re-plans a
 * block the reference elimination gives up on from every received repair, inside the same request, so
 * status is RECOVERED or SINGULAR where the call above reports REF_UB.  The mode belongs to the request,
 * not to the service: calls of both kinds may alternate on one service.  Arguments and the page-lock
 * check are the call's above; the re-plan's scratch counts against the worker's LDS, so a few large
 * blocks the call above takes are refused here (FECGPU_ERR_INVALID: take fecgpu_rlc_decode_host_full). */
int fecgpu_block_svc_rlc_decode_full(fecgpu_block_svc_t *svc, const void *src, const void *rep, void *dst,
                                     uint32_t k, uint32_t r, uint32_t symbol_size, const uint32_t *rep_seed,
                                     const uint64_t *src_present, const uint64_t *rep_present, uint8_t *status,
                                     uint64_t *recovered);
/* Row requests: one block with every row given by its address and its own length, so a caller whose
 * symbols lie in page-locked memory (a registered plugin arena) stages and copies nothing.  Semantics,
 * memory rules and clamping are those of fecgpu_rlc_encode_rows_fused, fecgpu_rlc_decode_rows_fused,
 * fecgpu_rlc_decode_rows_fused_full (full != 0), fecgpu_xor_encode_rows and fecgpu_xor_decode_rows applied
 * to one block of length blk_len (any value from 1 to 65532; it need not be a multiple of 4): a present
 * row is read for min(its length, blk_len) bytes; an absent row and a row of 0 bytes are never
 * dereferenced and may have address 0; a load may touch the aligned dword that holds a row's last byte
 * and nothing after it; each output row -- every repair (encode), the missing source's own entry of
 * src_rows (decode) -- receives exactly blk_len bytes by dword stores, then byte stores for the last 1-3
 * bytes, and no dword is read-modify-written; a block that is not RECOVERED writes no row.  One difference
 * from the launch forms: the worker fetches a block's rows while it plans the block, so the present rows
 * of an RLC block may be read before its status is known (a block the masks alone leave at NOTHING still
 * reads nothing) -- every present row of non-zero length must be readable, also a repair full mode would
 * not select.
 * All tables are plain host arrays, copied into the mailbox by the call: src_rows / src_len [k], rep_rows /
 * rep_len / rep_seed [r], the masks [2].  Row addresses are device addresses (what
 * fecgpu_host_device_address returns for page-locked host memory, or device memory), 4-byte aligned and
 * below 2^48.  status and recovered are host words.  Checked before anything is posted, FECGPU_ERR_INVALID
 * with a message and nothing written: the alignment and the 2^48 bound of every row that is read or
 * written, k in 1..128, r in 1..128, blk_len in 1..65532, and for the encodes src_len[j] <= blk_len (the
 * decodes truncate a received symbol longer than the block, as the reference does).  Refused with
 * FECGPU_ERR_INVALID like the packed calls, computed with L = blk_len rounded up to 4: RLC decode with
 * min(k, r) > 16 or knob plan non-zero, RLC rows beyond the worker's LDS, knob block_svc 0, a request
 * withdrawn at its deadline -- the caller then takes a launch form (fecgpu_rlc_encode_rows_fused_host
 * ...) with the same tables.  XOR blocks of any size are served: rows beyond the LDS go through it in
 * column slices.  Requests of every kind may alternate on one service.  Thread-safe. */
int fecgpu_block_svc_rlc_encode_rows(fecgpu_block_svc_t *svc, const uint64_t *src_rows, const uint32_t *src_len,
                                     const uint64_t *rep_rows, uint32_t blk_len, uint32_t k, uint32_t r,
                                     uint32_t fbn);
int fecgpu_block_svc_rlc_decode_rows(fecgpu_block_svc_t *svc, const uint64_t *src_rows, const uint32_t *src_len,
                                     const uint64_t *rep_rows, const uint32_t *rep_len, uint32_t blk_len, uint32_t k,
                                     uint32_t r, const uint32_t *rep_seed, const uint64_t *src_present,
                                     const uint64_t *rep_present, int full, uint8_t *status, uint64_t *recovered);
int fecgpu_block_svc_xor_encode_rows(fecgpu_block_svc_t *svc, const uint64_t *src_rows, const uint32_t *src_len,
                                     uint64_t rep_row, uint32_t blk_len, uint32_t k);
int fecgpu_block_svc_xor_decode_rows(fecgpu_block_svc_t *svc, const uint64_t *src_rows, const uint32_t *src_len,
                                     uint64_t rep_row, uint32_t blk_len, uint32_t k, const uint64_t *src_present,
                                     const uint64_t *rep_present, uint8_t *status, uint64_t *recovered);
/* worker generations launched so far (diagnostics: one per idle gap) */
uint64_t fecgpu_block_svc_launches(const fecgpu_block_svc_t *svc);
/* A call waits at most `deadline_us` (default 2000) for a worker to take its request.  Past it the
 * request is withdrawn on the spot unless a worker has claimed it (compare-and-swap on the request
 * number, against the worker's own claim): a withdrawn request is never served later, and the call
 * returns FECGPU_ERR_INVALID without waiting for the worker (it may be queued behind a long kernel),
 * so the caller takes the host path; for the next 50 ms every call returns FECGPU_ERR_INVALID at once.
 * A request a worker claimed before the deadline is being served and is waited for (the call
 * succeeds).  0: withdraw whatever is not done at the first check (tests). */
int fecgpu_block_svc_set_deadline(fecgpu_block_svc_t *svc, uint64_t deadline_us);
/* requests withdrawn at the deadline so far */
uint64_t fecgpu_block_svc_deadline_misses(fecgpu_block_svc_t *svc);
/* Diagnostics: the phases of the last served request.  out[0..3]: the worker's clock (s_memrealtime,
 * 100 MHz ticks) when it claimed the request, when the request was in LDS, when its rows were coded, and
 * just before it published `done`; out[4], out[5]: the host's clock (CLOCK_MONOTONIC, us) when the request
 * was posted and when the call saw it done.  Returns FECGPU_OK, or FECGPU_ERR_INVALID for NULL. */
int fecgpu_block_svc_last_stamps(fecgpu_block_svc_t *svc, uint64_t out[6]);
/* Whether a worker is running now (it ends by itself after 20 ms without a request, 50 ms in all):
 * 1 running, 0 not (or never launched), FECGPU_ERR_HIP if the last one ended in an error,
 * FECGPU_ERR_INVALID for NULL.  Lets a caller (a test) wait for the idle state instead of a time. */
int fecgpu_block_svc_worker_running(fecgpu_block_svc_t *svc);

/* FEC frames for a batch of repair symbols, ready for packet buffers (the block framework's
 * get_repair_payload_from_queue + write_fec_frame, block_framework_sender.h:100-133,
 * protoops/write_fec_frame.c; wire format in pquic_fec_frames.h).  Frame b*r + i, at
 * frames + (b*r + i) * frame_stride, is the 14-byte header {fin 1, data_length, offset 1,
 * repair FPID (fbn_b << 8) | i, nss, nrs} followed by the first data_length bytes of rep[b][i];
 * the rest of the slot is zeroed.  Device buffers; symbol_size and frame_stride multiples of 4,
 * frame_stride >= 14 + data_length. */
int fecgpu_write_repair_frames(const void *rep, uint64_t nblocks, uint32_t r, uint32_t symbol_size,
                               uint16_t data_length, uint32_t fbn_base, const uint32_t *fbn, uint8_t nss, uint8_t nrs,
                               void *frames, uint32_t frame_stride, void *stream);

/* Page-locked host memory for staging buffers (hipHostMalloc / hipHostFree), so callers in
 * C need no HIP headers.  NULL on failure. */
void *fecgpu_host_alloc(size_t bytes);
void fecgpu_host_free(void *p);
/* The host CPUs nearest the device ("local_cpulist" of its PCI function, e.g. "0-63,128-191"), for
 * placing the threads that feed it: page-locked rows read over PCIe from the device's own socket
 * avoid the cross-socket hop.  FECGPU_OK or an error. */
int fecgpu_device_local_cpus(int device, char *buf, size_t len);
/* Page-lock and map an existing host range (hipHostRegister, mapped) so the kernels read and write
 * it in place -- e.g. a FEC plugin instance's memory arena (picoquic_internal.h:576, char
 * memory[PLUGIN_MEMORY], carved into 2100-B slots by picoquic/memory.c:181-191), which holds every
 * symbol the framework hands over.  Unregister before the range is freed.  fecgpu_host_device_address
 * gives the device address of [p, p + bytes) when all of it lies in page-locked memory. */
int fecgpu_host_register(void *p, size_t bytes);
int fecgpu_host_unregister(void *p);
int fecgpu_host_device_address(const void *p, size_t bytes, uint64_t *dev);

/* Synthetic payload generator (bench/tests): byte o of dst = byte (o mod 8) of
 * splitmix64(seed + (o/8 + 1) * 0x9e3779b97f4a7c15), o counted from `offset`. */
int fecgpu_synth_fill(void *dst, uint64_t nbytes, uint64_t seed, uint64_t offset, void *stream);

/* Experiment knobs (A/B runs, cross-checks of alternative kernels in the tests).  Every knob has
 * a measured default and only these calls change it.  The engine reads no environment variable; the
 * batching adapter (pquic_fec_batch.h) reads three, once per batcher.  tools/ab_inproc.py maps the
 * FECGPU_* names of earlier rounds onto the knobs.  Names, accepted values and defaults (the engine's
 * table, FEC_KNOBS in fec_engine.hip):
 *   "plan"             0..5: 0 auto (default), 1 wave in LDS, 2 lane, 3 reg, 4 tile, 5 wave in registers
 *                      where it fits
 *   "interleave"       0..3, default 1: bit 0 interleaved block groups, bit 1 XCD-aware group order
 *   "group"            >= 0: 0 the per-shape group sizes (default), else a cap on blocks per group
 *   "enc_tile_rt"      0 the default tiling by r (default), else 1, 2, 4, 8 or 16 repairs per tile
 *   "enc_tile_waves"   0..4, default 0: waves per workgroup splitting a group's repairs (with enc_tile_rt)
 *   "enc_block_waves"  1 (default), 2 or 4: waves per workgroup of the register-prefetch encode, each
 *                      on its own block group
 *   "zc_read"          0/1, default 1: page-locked host buffers read in place; 0 staged by copies
 *   "ring"             2 (default) or 0: the LDS-ring data path of 16-repair / 16-unknown tiles on / off
 *   "window_sc"        0..2: window encode on the shared-coefficient kernel never (0), for overlapping
 *                      windows (1, default), wherever it applies (2)
 *   "min_groups"       >= 0, default 1024: batches with fewer block groups than this stream fewer blocks
 *                      per wave; 0 the per-shape group sizes at any batch size
 *   "chunk_waves"      0/1, default 1: symbols wider than one column chunk coded by 4-wave workgroups
 *                      over (block, chunk) items; 0 one wave per group
 *   "small_lds"        0/1, default 1: batches of <= 64 blocks with their rows staged in LDS; 0 the
 *                      bitsliced kernels
 *   "block_svc"        0/1, default 1: the resident single-block service; 0 refuses every request
 *   "ws_lds"           0/1, default 1: the recover data pass copies a group's plan records into LDS in
 *                      one round trip; 0 reads them in place
 *   "dec_waves"        0..8, default 0: at most n waves per SIMD for the register-prefetch recover tiles
 *   "yield_slice_kb"   0..1048576, default 2304: zero-copy bulk calls run in slices of this many KiB of
 *                      payload while the synchronous hooks are in use; 0 never slices
 *   "yield_depth"      1..16, default 16: slices in flight at most
 *   "yield_gate_us"    0..10000, default 0: a slice is held back at most this long while a hook request
 *                      is pending
 *   "yield_streams"    1..4, default 2: streams of the context the slices alternate over
 *   "yield_always"     0/1, default 0: slice even when no hook has run lately
 *   "yield_window_ms"  0..600000, default 100: the hooks count as in use for this long after a request
 * Returns FECGPU_OK, or FECGPU_ERR_INVALID for an unknown name or a value its knob does not accept. */
int fecgpu_set_knob(const char *name, int value);
int fecgpu_get_knob(const char *name, int *value);

/* Per-process counters, the analogue of the reference's per-pluglet count/time
 * (picoquic/ubpf.c:302-319 under DEBUG_PLUGIN_EXECUTION_TIME). */
typedef struct {
    uint64_t encode_calls, encode_blocks;
    uint64_t decode_calls, decode_blocks;
    /* host path: page-locked buffers found in the library's registry of its own fecgpu_host_alloc /
     * fecgpu_host_register ranges, and those that needed a hipPointerGetAttributes query instead */
    uint64_t pinned_registry_hits, pinned_registry_misses;
    /* zero-copy bulk calls while the synchronous hooks are in use: slices launched, and slices held back
     * until a pending hook request had finished (host_path.hip, Pacer) */
    uint64_t yield_slices, yield_waits;
} fecgpu_stats_t;
void fecgpu_get_stats(fecgpu_stats_t *out);

#ifdef __cplusplus
}
#endif
#endif
