/*
 * include/pquic_fec_protoops.h -- drop-in protocol operations for PQUIC's plugins/fec
 * scheme hooks, backed by the MI355X engine (include/fecgpu.h).
 *
 * The reference ships three scheme pluglets per FEC scheme, compiled to eBPF and run by
 * uBPF, declared by the manifests plugins/fec/fec_scheme_rlc_gf256.plugin:1-3 and
 * plugins/fec/fec_scheme_xor.plugin:1-3:
 *
 *   protoop id                    reference pluglet (RLC / XOR)                      replaced by
 *   create_fec_schemes            create_rlc_fec_scheme_gf256.c:46-59 / create_xor_fec_scheme.c:4-9
 *                                                                 pquic_fec_{rlc,xor}_create_fec_schemes
 *   fec_generate_repair_symbols   rlc_fec_scheme_generate_gf256.c:24-77 / xor_fec_scheme_generate.c:41-78
 *                                                                 pquic_fec_{rlc,xor}_generate_repair_symbols
 *   fec_recover                   rlc_fec_scheme_gf256.c:134-251 / xor_fec_scheme.c:41-74
 *                                                                 pquic_fec_{rlc,xor}_recover
 *
 * Every function has the reference's protocol_operation signature
 * (picoquic/picoquic_internal.h:582: protoop_arg_t op(picoquic_cnx_t *)), reads its inputs
 * with get_cnx(cnx, AK_CNX_INPUT, i), writes outputs with set_cnx(cnx, AK_CNX_OUTPUT, i, v)
 * and returns the same codes as the pluglet it replaces.  Repair / recovered symbols are
 * allocated with the caller's my_malloc, exactly like malloc_repair_symbol /
 * malloc_source_symbol (plugins/fec/fec.h:201-231), so the framework frees them as before.
 *
 * picoquic's accessors are bound at run time (pquic_fec_bind_host) so that this library
 * does not link against picoquic; see INTEGRATION.md for the registration stub.
 */
#ifndef PQUIC_FEC_PROTOOPS_H
#define PQUIC_FEC_PROTOOPS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- picoquic plugin ABI (picoquic/picoquic.h:333, getset.h:11,339-341) ---- */
typedef uint64_t protoop_arg_t;
typedef struct st_picoquic_cnx_t picoquic_cnx_t;
typedef uint16_t access_key_t;
#define PQUIC_AK_CNX_INPUT  0x00
#define PQUIC_AK_CNX_OUTPUT 0x01
#define PQUIC_ERROR_MEMORY  0x405   /* PICOQUIC_ERROR_MEMORY = PICOQUIC_ERROR_CLASS + 5 */
#define PQUIC_FEC_MAX_SYMBOLS_PER_BLOCK 100   /* plugins/fec/fec.h:8 */

/* ---- layout-compatible view of the reference FEC data model (plugins/fec/fec.h:44-130),
 *      x86-64 SysV; sizes pinned by tests/golden/layout.json ---- */
typedef union {
    uint32_t raw;
    struct __attribute__((__packed__)) { uint8_t symbol_number; uint32_t fec_block_number : 24; } f;
} pquic_source_fpid_t;

typedef union {
    uint64_t raw;
    struct __attribute__((__packed__)) {
        pquic_source_fpid_t source_fpid;   /* symbol_number | fec_block_number << 8 */
        uint32_t fec_scheme_specific;
    } f;
} pquic_repair_fpid_t;

typedef struct {
    pquic_repair_fpid_t fpid;            /* repair_fec_payload_id */
    uint16_t data_length : 15;
    uint8_t *data;
} pquic_repair_symbol_t;

typedef struct {
    pquic_source_fpid_t fpid;            /* source_fec_payload_id (fec_block_offset, fbn) */
    uint16_t data_length : 15;
    uint8_t *data;
} pquic_source_symbol_t;

typedef struct __attribute__((__packed__)) {
    uint32_t fec_block_number;
    uint8_t total_source_symbols;
    uint8_t total_repair_symbols;
    uint8_t current_source_symbols;
    uint8_t current_repair_symbols;
    pquic_source_symbol_t *source_symbols[PQUIC_FEC_MAX_SYMBOLS_PER_BLOCK];
    pquic_repair_symbol_t *repair_symbols[PQUIC_FEC_MAX_SYMBOLS_PER_BLOCK];
} pquic_fec_block_t;

/* ---- host accessors (picoquic/getset.h:28,38; picoquic/memory.h:6,8) ---- */
typedef struct {
    protoop_arg_t (*get_cnx)(picoquic_cnx_t *cnx, access_key_t ak, uint16_t param);
    void (*set_cnx)(picoquic_cnx_t *cnx, access_key_t ak, uint16_t param, protoop_arg_t val);
    void *(*my_malloc)(picoquic_cnx_t *cnx, unsigned int size);
    void (*my_free)(picoquic_cnx_t *cnx, void *ptr);
    /* optional: the skip_frame protoop (helper_skip_frame, plugins/helpers.h:234-245); needed
     * only by pquic_fec_packet_payload_to_source_symbol */
    int (*skip_frame)(picoquic_cnx_t *cnx, uint8_t *bytes, size_t bytes_max, size_t *consumed, int *pure_ack);
} pquic_fec_host_api_t;

/* Bind picoquic's accessors; returns 0.  Until bound every protoop returns
 * PQUIC_FEC_ERR_UNBOUND.  `device` selects the HIP device the schemes use. */
int pquic_fec_bind_host(const pquic_fec_host_api_t *api, int device);
#define PQUIC_FEC_ERR_UNBOUND 0x41B     /* PICOQUIC_ERROR_UNEXPECTED_ERROR */

/* Scheme object handed out by create_fec_schemes (outputs 0 and 1, like the reference's
 * rlc_gf256_fec_scheme_t*).  Opaque to the framework. */
typedef struct pquic_fec_scheme pquic_fec_scheme_t;

/* ---- the protocol operations ---- */
protoop_arg_t pquic_fec_rlc_create_fec_schemes(picoquic_cnx_t *cnx);
protoop_arg_t pquic_fec_rlc_generate_repair_symbols(picoquic_cnx_t *cnx);
protoop_arg_t pquic_fec_rlc_recover(picoquic_cnx_t *cnx);
protoop_arg_t pquic_fec_xor_create_fec_schemes(picoquic_cnx_t *cnx);
protoop_arg_t pquic_fec_xor_generate_repair_symbols(picoquic_cnx_t *cnx);
protoop_arg_t pquic_fec_xor_recover(picoquic_cnx_t *cnx);

/* How pquic_fec_rlc_recover solves a block.  0 (default): the reference's elimination, bit for bit -- the
 * first n received repairs, one sort, no re-pivoting; a block it gives up on (a zero pivot, where the
 * reference reads out of bounds) returns 0 with nothing inserted and counts in ref_ub_blocks.  1: full
 * rank -- every block the received repairs determine is recovered, through a later repair where the first
 * n are dependent; the recovered symbols have the reference's FPIDs and lengths, so the frameworks see no
 * difference but more recovered symbols.  A block they do not determine returns what a given-up block
 * returns in mode 0, inserts nothing and counts in pquic_fec_singular_blocks(); ref_ub_blocks stays 0.
 * XOR is not affected.  Process-wide, like pquic_fec_bind_host; takes effect from the next call.
 * Returns 0, or -1 for any other value, and for mode 1 against an engine library without the full-rank
 * entry points (the mode then stays as it was). */
int pquic_fec_set_recover_mode(int mode);
int pquic_fec_get_recover_mode(void);
/* Blocks full-rank recovery found undetermined so far, in the protocol operations and in the batching
 * adapter's completions alike. */
uint64_t pquic_fec_singular_blocks(void);

/* Where the generate and recover operations (RLC and XOR) find their symbols.  0 (default): every symbol
 * is copied into page-locked staging rows and every result is copied out of them.  1, in place: a symbol
 * whose data is 4-byte aligned and lies in page-locked memory the engine knows (fecgpu_host_device_address:
 * a range registered below or by a batcher, pquic_fec_batch_register_arena) is handed to the engine by its
 * address and its own data_length, and results are allocated before the engine call and written where
 * they lie; any other symbol still goes through a staging row, so one block may mix both kinds.  The
 * block goes to the resident block service's row requests first (XOR included) and, where the service
 * refuses, through the launch forms on the same tables.  Returns, bytes, lengths, FPIDs, counters and the
 * recover mode behave as with 0.  Process-wide; takes effect from the next call.  Returns 0, or -1 for
 * any other value, and for 1 against an engine library without the row requests (the mode then stays as
 * it was). */
int pquic_fec_set_hooks_in_place(int on);
int pquic_fec_get_hooks_in_place(void);
/* Page-locks [base, base + bytes) -- the allocator's arena -- and makes it known to the engine, for an
 * integrator who uses the protocol operations without a batcher: thin wrappers over fecgpu_host_register
 * / fecgpu_host_unregister, 0 or -1.  A range a batcher has registered (pquic_fec_batch_register_arena)
 * is page-locked already and needs no second registration. */
int pquic_fec_register_heap(void *base, size_t bytes);
int pquic_fec_unregister_heap(void *base);
/* In-place mode's counters: out[0] rows handed over where they lie, out[1] rows that went through a
 * staging row, out[2] calls the block service's worker served, out[3] calls that took a launch form. */
void pquic_fec_hook_rows_stats(uint64_t out[4]);

/* A span of the sliding-window receiver's stream, for span recovery (opt-in, beyond the reference): the joint
 * decode of the framework's overlapping windows (fecgpu_rlc_span_decode, fecgpu.h).  K consecutive symbols of
 * one connection's stream -- ids base_id .. base_id + K - 1 modulo 2^32 -- with the received ones in src[] and
 * R received repair symbols, each with the window it protects: repair i covers the nss[i] symbols from stream
 * id first_id[i] and is seeded by its own FPID, as fec_recover seeds every equation. */
typedef struct {
    uint32_t base_id;                    /* stream id of column 0 (ids modulo 2^32) */
    uint32_t K, R;                       /* 1..128 columns, 1..128 received repairs */
    pquic_source_symbol_t *const *src;   /* [K], NULL where the symbol is missing */
    pquic_repair_symbol_t *const *rep;   /* [R], none NULL; seed = its FPID as in fec_recover */
    const uint32_t *first_id;            /* [R] window start of repair i (fec_scheme_specific) */
    const uint8_t *nss;                  /* [R] window length of repair i */
} pquic_fec_span_t;
/* Span recovery, blocking (one span per call, serialised like the operations above): every missing column
 * the span's repairs determine is recovered, through neighbouring windows where no window alone would do.
 * The semantics are those of a batcher span completion (pquic_fec_batch_recover_span, pquic_fec_batch.h), so
 * one span gives the same symbols through either path.
 * Returns PQUIC_FEC_ERR_UNBOUND with *nrecovered = 0 and nothing allocated: before pquic_fec_bind_host, for a
 * NULL argument or table entry, K or R outside 1..128, a repair with nss == 0 or a window that leaves [0, K)
 * (column offsets are first_id[i] - base_id modulo 2^32), and against an engine library without
 * fecgpu_rlc_span_decode_rows_fused_host.  (No symbol is longer than 32767 bytes: data_length has 15 bits.)  A span with no missing column returns 0
 * with nothing recovered.
 * Otherwise one source symbol is allocated through the bound allocator for every missing column:
 * data_length = the span's length (the largest data_length among its repairs; a received source counts for
 * at most that many bytes), fpid.raw = base_id + column.  A symbol whose data is 4-byte aligned and lies in
 * page-locked memory the engine knows (pquic_fec_register_heap, a batcher's arena) is read or written where
 * it lies, for its own length; any other goes through a staging row -- whatever pquic_fec_set_hooks_in_place
 * says, which keeps governing generate and recover only; pquic_fec_hook_rows_stats counts these rows too.
 * The span is decoded by one fecgpu_rlc_span_decode_rows_fused_host call (one kernel launch for every shape
 * whose plan fits LDS, fecgpu.h).  On success the return is 0, recovered[c] is the symbol of every column c of
 * the engine's recovered[] mask (a determined source that is all zero is not handed over) and NULL elsewhere,
 * *nrecovered their number; every other pre-allocation has been freed first, in column order; the symbols
 * are the caller's.  A span with losses and repairs that determines nothing returns 0 with *nrecovered = 0
 * and counts in pquic_fec_singular_blocks().  recover_calls and recovered_symbols count as for recover.  On
 * an engine error every pre-allocation is freed, errors counts and PQUIC_FEC_ERR_UNBOUND is returned. */
protoop_arg_t pquic_fec_rlc_recover_span(picoquic_cnx_t *cnx, const pquic_fec_span_t *sp,
                                         pquic_source_symbol_t **recovered /* [sp->K] */, uint32_t *nrecovered);

/* packet_payload_to_source_symbol (protoops/packet_payload_to_source_symbol.c:6-36, manifest
 * fec_core.plugin:20): inputs [0] payload bytes, [1] symbol buffer, [2] payload length,
 * [3] packet number; returns the symbol length, PQUIC_ERROR_MEMORY for a NULL buffer, or
 * PQUIC_FEC_ERR_UNBOUND without a bound skip_frame.  The pluglet's store to
 * bpf_state.current_symbol_length is not reproduced: both callers overwrite or never read it
 * (incoming_encrypted.c:29-33, schedule_frames_on_path.c:47). */
protoop_arg_t pquic_fec_packet_payload_to_source_symbol(picoquic_cnx_t *cnx);

/* Counters of adapter activity (calls, blocks the reference would have crashed on; calls whose request
 * the resident block service withdrew at its deadline, which then took the launch path --
 * fecgpu_block_svc_set_deadline). */
typedef struct {
    uint64_t generate_calls, recover_calls, recovered_symbols, ref_ub_blocks, errors;
    uint64_t svc_deadline_misses;
} pquic_fec_protoop_stats_t;
void pquic_fec_protoop_stats(pquic_fec_protoop_stats_t *out);

/* Layout self-description for tests: {sizeof block, source, repair, offsetof source_symbols,
 * repair_symbols, source data, repair data, sizeof repair fpid}. */
int pquic_fec_layout(uint64_t out[8]);

#ifdef __cplusplus
}
#endif
#endif
