/*
 * pquic_fec_batch.h -- batching adapter for PQUIC's block FEC framework.
 *
 * The reference runs fec_generate_repair_symbols / fec_recover synchronously, one block per
 * protocol-operation call (block_framework_sender.h:175-203 generate_and_queue_repair_symbols;
 * block_framework_receiver.h:29-80 via fec_protoops.h:215-246 recover_block).  On a GPU a
 * single block is pure launch and PCIe latency, so this adapter queues blocks from any number
 * of connections into per-(operation, scheme, k, r) batches in page-locked memory and runs a
 * batch through the device engine when it is full or when its oldest block has waited
 * `max_delay_us` (the latency cap).  A worker thread runs the engine (H2D, kernels, D2H
 * overlapped on HIP streams) while the caller keeps queueing.
 *
 * Completion has exactly the synchronous operation's effect: the repair symbols (or
 * recovered source symbols) are allocated with the bound host allocator
 * (pquic_fec_bind_host), written into the caller's fec_block_t with the reference's FPIDs,
 * lengths and counters, and `done(user, fb, ret)` receives the value the protocol operation
 * would have returned.  Completions run on the caller's thread inside pquic_fec_batch_poll /
 * pquic_fec_batch_drain, never on the worker, because picoquic's allocator and connection
 * state are single-threaded (picoquic/memory.c, plugin.c:1357-1360).
 *
 * The caller keeps `fb` (and its symbols) alive and unmodified until `done` runs for it.
 */
#ifndef PQUIC_FEC_BATCH_H
#define PQUIC_FEC_BATCH_H

#include <stddef.h>
#include <stdint.h>

#include "pquic_fec_protoops.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pquic_fec_batcher pquic_fec_batcher_t;

typedef struct {
    int device;              /* HIP device */
    uint32_t batch_blocks;   /* a queue is flushed when it holds this many blocks (>= 1) */
    uint32_t max_delay_us;   /* ... or when its oldest block has waited this long (poll) */
    uint32_t max_symbol;     /* largest symbol length accepted (<= 32767, fec.h:95,109) */
    int nstreams;            /* HIP streams the engine pipelines a batch over (>= 1) */
    uint32_t poll_blocks;    /* poll completes at most this many blocks per call (0: every finished one);
                              * a sender's event loop that polls between submissions then frees and
                              * reallocates symbols in small interleaved runs, so its allocator's free
                              * list stays in cache */
} pquic_fec_batch_cfg_t;

/* Called once per submitted block, on the caller's thread (see above). */
typedef void (*pquic_fec_block_done_fn)(void *user, pquic_fec_block_t *fb, protoop_arg_t ret);

typedef struct {
    uint64_t submitted, completed;  /* blocks */
    uint64_t batches;               /* engine calls */
    uint64_t flushed_full, flushed_deadline, flushed_drain;
    uint64_t immediate;             /* blocks completed at submit (preconditions failed) */
    uint64_t engine_errors;
    uint64_t windows, window_rows;  /* window blocks coded from shared streams; stream rows laid out for them */
    uint64_t engine_us, stage_us;   /* thread time in engine calls / in stager work items (all threads) */
    uint64_t complete_us;           /* caller-thread time in completions (poll / drain) */
    uint64_t rows_in_place;         /* symbol rows the kernels read or wrote where they lie (registered arenas) */
    uint64_t rows_staged;           /* symbol rows copied through the page-locked staging rows instead */
    uint64_t jobs_allocated;        /* batch jobs (page-locked queue buffers) allocated on the caller's thread */
    uint64_t job_alloc_us;          /* caller-thread time in those allocations */
    uint64_t deadline_holds;        /* polls that kept an overdue queue open: no idle job for its successor while
                                     * two or more were in flight (flushed at the first poll with one back) */
    uint64_t spans, span_symbols;   /* spans decoded by span jobs (pquic_fec_batch_recover_span); source symbols
                                     * they handed over */
} pquic_fec_batch_stats_t;

/* NULL on failure (bad configuration, no device, out of pinned memory).
 * The adapter reads five environment variables, once per batcher, here (a value below the minimum
 * counts as unset, one above the maximum as the maximum):
 *   PQUIC_FEC_BATCH_STAGERS   copy threads, 1..16; default half the CPUs of the process's share, at least 2
 *   PQUIC_FEC_BATCH_ENGINES   engine threads, each with its own host context and streams, 1..4; default 2
 *   PQUIC_FEC_BATCH_PREFETCH  blocks ahead a completion prefetches the symbols it hands over, 0..64
 *                             (0: off); default 8
 *   PQUIC_FEC_BATCH_FULL_RANK 0 or 1: the batcher starts in full-rank mode (pquic_fec_batch_set_full_rank);
 *                             default 0; ignored against an engine library without the full-rank entry points
 *   PQUIC_FEC_BATCH_WINDOW_MIXED 0 or 1: the batcher starts with mixed window jobs
 *                             (pquic_fec_batch_set_window_mixed); default 0; ignored against an engine library
 *                             without fecgpu_rlc_window_encode_rows_var_host */
pquic_fec_batcher_t *pquic_fec_batcher_create(const pquic_fec_batch_cfg_t *cfg);
/* Drains (completing every queued block) and frees. */
void pquic_fec_batcher_destroy(pquic_fec_batcher_t *b);

/* Register a host memory range that holds symbols -- a FEC plugin instance's memory arena
 * (picoquic_internal.h:576, char memory[PLUGIN_MEMORY], carved into 2100-B slots by
 * picoquic/memory.c:181-191, registered once after init_memory_management, memory.c:254).  Every
 * connection owns its plugin instances (plugin.c:835, 946-950), so a process registers one arena per
 * connection: any number of them, kept sorted and looked up by binary search, registered and
 * unregistered while batches run (call from the thread that submits).  It is page-locked and mapped
 * (fecgpu_host_register) until unregistered or the batcher is destroyed.  RLC generate batches then
 * read source symbols and write repair symbols in it directly, and RLC recover batches read the received
 * sources and repairs in it and write each recovered source into a symbol allocated for it at submission
 * (through the bound allocator, so in the connection's arena), instead of copying rows through staging
 * rows.  Symbols need not be as long as the stride (max_symbol padded to 4) or as the block: a batch with
 * ragged blocks hands every symbol over with its own length (fecgpu_rlc_encode_rows_len_host /
 * fecgpu_rlc_decode_rows_len_host), so only the bytes that exist cross PCIe, repairs and recovered
 * sources receive exactly the block's length, and only symbols outside every registered range are
 * staged.  (Against an engine library without those two entry points ragged blocks are staged,
 * zero-padded to the stride.)  XOR batches use the range the same way, through
 * fecgpu_xor_encode_rows_host / fecgpu_xor_decode_rows_host (one pass, a length per row, whatever the
 * lengths): generate reads the sources and writes the one repair where its symbol lies; recover reads
 * the received sources and the repair and writes the recovered source into the symbol allocated at
 * submission for the last missing index, with the XOR operation's FPID (fec_block_number << 8 | j), return
 * value and counters (current_source_symbols stays as it was).  (Against an engine library without those
 * two entry points XOR blocks are staged, packed and zero-padded.)  Window batches
 * (pquic_fec_batch_generate_window) use the range too, through fecgpu_rlc_window_encode_rows_host: every
 * stream symbol in it is handed over once, by address and data_length, the device builds the de-duplicated
 * stream from those rows, and every repair symbol in it is written where it lies for the window's length;
 * only symbols outside every registered range go through staging rows.  (Against an engine library without
 * that entry point the stream is copied into page-locked rows and the repairs are copied out.)
 * Returns 0, or -1 (NULL / empty range, overlap with a registered range, registration failure). */
int pquic_fec_batch_register_heap(pquic_fec_batcher_t *b, void *base, size_t bytes);
/* Unregister the range registered at `base` (a connection closing).  No block whose symbols lie in it
 * may still be queued: the caller has had every done() for them.  Returns 0 or -1. */
int pquic_fec_batch_unregister_heap(pquic_fec_batcher_t *b, void *base);

/* Queue fec_generate_repair_symbols (xor_scheme = 0: RLC-GF(256), 1: XOR) for `fb`, whose
 * totals are set as the block framework sets them before the call
 * (block_framework_sender.h:184-185).  `now_us` starts the block's latency clock.
 * Returns 0 when accepted -- `done` is then called exactly once, possibly before this returns
 * when the reference's preconditions fail -- or -1 (NULL argument, symbol longer than
 * max_symbol, allocation failure), in which case `done` is never called. */
int pquic_fec_batch_generate(pquic_fec_batcher_t *b, picoquic_cnx_t *cnx, pquic_fec_block_t *fb, int xor_scheme,
                             uint64_t now_us, pquic_fec_block_done_fn done, void *user);
/* Queue fec_generate_repair_symbols (RLC-GF(256)) for a window block of the sliding-window sender
 * (window_framework_sender.h:209-260: malloc_fec_block(cnx, 0) at :215, the symbols in flight chosen by
 * window_select_symbols_to_protect, the generate call at :235).  Same contract and result as
 * pquic_fec_batch_generate; in addition the batch lays each connection's symbols out once, as one stream of
 * rows, for all the windows that share them (copied into page-locked rows, or with a registered heap handed
 * over where they lie) and codes the windows together (every window is block number 0, so they share
 * their coefficients).  Windows from one connection should arrive in sending order, as the sender
 * produces them; a block with a non-zero block number is queued as an ordinary block. */
int pquic_fec_batch_generate_window(pquic_fec_batcher_t *b, picoquic_cnx_t *cnx, pquic_fec_block_t *fb,
                                    uint64_t now_us, pquic_fec_block_done_fn done, void *user);
/* Queue fec_recover for `fb` (the receiver's block copy, fec_protoops.h:220-222). */
int pquic_fec_batch_recover(pquic_fec_batcher_t *b, picoquic_cnx_t *cnx, pquic_fec_block_t *fb, int xor_scheme,
                            uint64_t now_us, pquic_fec_block_done_fn done, void *user);

/* Span recovery (opt-in, beyond the reference): the joint decode of the sliding-window framework's
 * overlapping windows (fecgpu_rlc_span_decode, fecgpu.h).  A span is K consecutive symbols of one connection's
 * stream -- ids base_id .. base_id + K - 1 modulo 2^32 -- with the received ones in src[] and R received repair
 * symbols, each with the window it protects: repair i covers the nss[i] symbols from stream id first_id[i]
 * (its fec_scheme_specific field, window_framework_receiver.h:60-86) and is seeded by its own FPID
 * (rep[i]->fpid.f.source_fpid.raw), as fec_recover seeds every equation.  Every missing column the repairs
 * determine is recovered, through neighbouring windows where no window alone would do. */
/* (pquic_fec_span_t: pquic_fec_protoops.h, which the blocking call pquic_fec_rlc_recover_span shares) */
/* Called once per accepted span, on the caller's thread.  recovered[c] is the symbol recovered for column c or
 * NULL; the array is the batcher's and valid during the call, the symbols are the caller's from then on. */
typedef void (*pquic_fec_span_done_fn)(void *user, const pquic_fec_span_t *sp,
                                       pquic_source_symbol_t *const *recovered /* [K], NULL where none */,
                                       uint32_t nrecovered, protoop_arg_t ret);
/* Queue a span.  The contract is pquic_fec_batch_recover's: the caller keeps `sp`, its arrays and its symbols
 * alive and unmodified until `done` runs, which happens exactly once, from poll or drain, in flush and
 * submission order with the other completions.  Column offsets are first_id[i] - base_id modulo 2^32.
 * Returns -1 -- `done` never runs -- for a NULL argument or table entry, K or R outside 1..128, a repair with
 * nss == 0 or a window that leaves [0, K), a symbol longer than max_symbol, an allocation failure, and against
 * an engine library without fecgpu_rlc_span_decode_rows_fused_host.  A span with no missing column completes
 * inside the call with nothing recovered (stats.immediate).
 * At submission one source symbol is allocated through the bound allocator for every missing column, so in
 * the connection's arena: data_length = the span's length (the largest data_length among its repairs; a
 * received source counts for at most that many bytes), fpid.raw = base_id + column.  The kernel writes the
 * recovered bytes into them where they lie when they are in a registered heap, as it reads the received rows
 * there, each for its own length; rows outside every heap go through the job's staging rows and recovered
 * ones of that kind are copied into their symbols at completion (rows_in_place / rows_staged count both).
 * At completion the columns of the engine's recovered[] mask are handed over -- a determined source that is
 * all zero is not, the zero rule of every other path -- and every other pre-allocation is freed first, in
 * column order, as recover jobs free theirs.  ret is 0 whenever the engine call succeeded: a span whose
 * repairs determine nothing has nrecovered == 0 and, where it had losses and repairs, counts in
 * pquic_fec_singular_blocks(); an engine error gives PQUIC_FEC_ERR_UNBOUND as for recover jobs.
 * Spans of different widths share jobs: a span is padded to its queue's shape, K to 64 or 128 columns (a
 * padding column is present with length 0 and no repair covers it) and R to 8, 32 or 128 slots (a padding slot
 * is absent), six queues in all; batch_blocks, max_delay_us, poll_blocks, the provisioner and the small-job
 * rule apply to them as to recover jobs.  With the engine's knob span_compact (default 1) the data pass skips
 * every column no unknown depends on, the padding included. */
int pquic_fec_batch_recover_span(pquic_fec_batcher_t *b, picoquic_cnx_t *cnx, const pquic_fec_span_t *sp,
                                 uint64_t now_us, pquic_fec_span_done_fn done, void *user);

/* Full-rank recovery for the RLC recover jobs of this batcher (on != 0; 0: the reference's elimination, the
 * default).  A full-rank job recovers every block its received repairs determine -- also where the reference
 * gives up on a zero pivot, and through repairs past the first n -- by fecgpu_rlc_decode_rows_fused_host_full
 * (ragged blocks in place), fecgpu_rlc_decode_rows_host_full (whole blocks in place) or
 * fecgpu_rlc_decode_host_full (staged); a block they do not determine completes with nothing recovered and
 * is counted by pquic_fec_singular_blocks().  Pre-allocation at submission, the order in which unrecovered
 * pre-allocations are freed, completion order and FPIDs are the same in both modes; generate and XOR jobs
 * are not affected.  Call from the submitting thread.  Returns 0, or -1 while any block is queued or in
 * flight (drain first) and against an engine library without the three entry points. */
int pquic_fec_batch_set_full_rank(pquic_fec_batcher_t *b, int on);

/* Mixed window jobs (on != 0; 0, the default: a window queue per (k, r), nothing changes).  The window sender
 * protects whatever is in flight, 1 to 30 symbols, a count that changes with every ACK and every send
 * (window_protect_all_inflight_source_symbols.c:12-23), so under the default key its windows spread over up to
 * 30 queues per r, each flushed on its deadline with a fraction of a batch, and a connection's run of stream
 * rows ends at every change of length.  With mixed jobs pquic_fec_batch_generate_window queues a window under
 * (kclass, r), kclass the smallest of 16, 32, 64 and 128 that holds total_source_symbols; the job records each
 * window's length, matches and extends a connection's run with it (looking back at most kclass rows), and runs
 * through fecgpu_rlc_window_encode_rows_var_host, always on rows by address: symbols and repairs in a
 * registered heap where they lie, any other through the job's staging rows (there is no packed staged form; a
 * job whose windows all have one length runs through fecgpu_rlc_window_encode_rows_host for that length).  r
 * stays in the key: it differs from the controller's value only for windows shorter than n - k.  The 2 GiB
 * test of pquic_fec_batch_generate_window (with kclass in it), buffer sizing, the provisioner, completion order
 * (submission order), the FPIDs 0..r-1 and `done` exactly once are unchanged.  Call from the submitting
 * thread.  Returns 0, or -1 while any block is queued or in flight (drain first) and against an engine library
 * without fecgpu_rlc_window_encode_rows_var_host. */
int pquic_fec_batch_set_window_mixed(pquic_fec_batcher_t *b, int on);

/* Flushes every queue that is full or past its deadline at `now_us`, then runs `done` for
 * the blocks whose batch has finished: all of them, or at most cfg.poll_blocks.  Batches complete
 * in the order they were flushed (a finished batch waits for the ones flushed before it), and the
 * blocks of a batch in submission order, so the blocks of one queue -- one (operation, scheme, k, r)
 * -- complete in submission order, as the synchronous operation completes them one by one; a block
 * whose preconditions fail completes inside its submission call.  Non-blocking.  Returns the number
 * of completions. */
int pquic_fec_batch_poll(pquic_fec_batcher_t *b, uint64_t now_us);
/* Flushes everything and waits until every queued block has completed.  Returns the number
 * of completions. */
int pquic_fec_batch_drain(pquic_fec_batcher_t *b);

void pquic_fec_batch_get_stats(const pquic_fec_batcher_t *b, pquic_fec_batch_stats_t *out);

#ifdef __cplusplus
}
#endif
#endif
