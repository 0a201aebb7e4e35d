/*
 * pquic_amd/csrc/protoops.c -- PQUIC protocol operations for the FEC scheme hooks
 * (include/pquic_fec_protoops.h), host side in C like the reference pluglets.
 *
 * Each operation reads the fec_block_t the framework passes in, stages its symbols into a
 * zero-padded fixed-size row layout, runs the device engine through the host-resident
 * entry points of include/fecgpu.h (one block per call, synchronous like the reference),
 * and writes results back into the block with the caller's allocator.  With
 * pquic_fec_set_hooks_in_place(1) the symbols that lie in page-locked memory are handed over by address
 * instead and the results are written where they lie (the in-place mode below).  The arithmetic
 * itself never runs on the CPU: if no gfx950 device is usable the operation fails with an
 * error code instead of computing.
 */
#include "pquic_fec_protoops.h"
#include "pquic_fec_frames.h"

#include <pthread.h>
#include <stdlib.h>
#include <string.h>

#include "fec_core.h"
#include "fecgpu.h"

_Static_assert(sizeof(pquic_source_fpid_t) == 4, "source_fpid_t is 4 bytes (fec.h:44-50)");
_Static_assert(sizeof(pquic_repair_fpid_t) == 8, "repair_fpid_t is 8 bytes (fec.h:63-75)");
_Static_assert(sizeof(pquic_source_symbol_t) == 16, "source_symbol_t layout (fec.h:104-114)");
_Static_assert(sizeof(pquic_repair_symbol_t) == 24, "repair_symbol_t layout (fec.h:91-102)");
_Static_assert(sizeof(pquic_fec_block_t) == 1608, "fec_block_t layout (fec.h:121-130)");

#define RLC_MAGIC 0x524c4347u /* "RLCG" */

struct pquic_fec_scheme {
    uint32_t magic;
    uint32_t device;
};

pquic_fec_host_api_t g_fec_api;
int g_fec_bound;
pquic_fec_protoop_stats_t g_fec_stats;
uint64_t g_fec_singular_blocks;
static int g_device;
/* Full-rank recovery is optional: an engine without its entry points (the CPU stand-in of the sanitizer
 * builds) leaves these NULL and mode 1 is refused. */
#pragma weak fecgpu_block_svc_rlc_decode_full
#pragma weak fecgpu_rlc_decode_host_full
static int g_recover_mode; /* 0 reference, 1 full rank (pquic_fec_set_recover_mode), under g_mu */
/* In-place mode is optional in the same way: it needs the block service's row requests and the launch
 * forms on row tables they fall back to. */
#pragma weak fecgpu_block_svc_rlc_encode_rows
#pragma weak fecgpu_block_svc_rlc_decode_rows
#pragma weak fecgpu_block_svc_xor_encode_rows
#pragma weak fecgpu_block_svc_xor_decode_rows
#pragma weak fecgpu_rlc_encode_rows_fused_host
#pragma weak fecgpu_rlc_decode_rows_fused_host
#pragma weak fecgpu_rlc_decode_rows_fused_host_full
#pragma weak fecgpu_xor_encode_rows_host
#pragma weak fecgpu_xor_decode_rows_host
/* And span recovery: without the span decode on rows pquic_fec_rlc_recover_span refuses every span. */
#pragma weak fecgpu_rlc_span_decode_rows_fused_host
static int g_in_place;          /* pquic_fec_set_hooks_in_place, under g_mu */
static uint64_t g_row_stats[4]; /* rows in place, rows staged, calls the worker served, calls launched; under g_mu */
static fecgpu_host_ctx_t *g_ctx;
/* the resident single-block service (fecgpu_block_svc_*): one block per call without a kernel launch;
 * calls it refuses (block too large for it, knob off) take the host path */
static fecgpu_block_svc_t *g_svc;
static int g_svc_failed;
static pthread_mutex_t g_mu = PTHREAD_MUTEX_INITIALIZER;

/* Per-call staging, page-locked (fecgpu_host_alloc) and grown on demand: the engine's host path
 * then runs zero-copy -- the kernels read the staged rows and write repairs / recovered rows and
 * the small per-block arrays (seeds, masks, status) in place over PCIe -- so a one-block call is
 * launches plus one synchronisation, with no copy stages. */
static uint8_t *g_src, *g_rep;
static size_t g_src_cap, g_rep_cap;
typedef struct {
    uint32_t seeds[PQUIC_FEC_MAX_SYMBOLS_PER_BLOCK];
    uint64_t sp[2], rp[2], rec[2];
    uint8_t st;
} aux_t;
static aux_t *g_aux;

int pquic_fec_bind_host(const pquic_fec_host_api_t *api, int device) {
    pthread_mutex_lock(&g_mu);
    if (api) {
        g_fec_api = *api;
        g_fec_bound = api->get_cnx && api->set_cnx && api->my_malloc && api->my_free;
    } else {
        g_fec_bound = 0;
    }
    if (g_ctx && g_device != device) {
        fecgpu_host_ctx_destroy(g_ctx);
        g_ctx = NULL;
    }
    if (g_svc && g_device != device) {
        fecgpu_block_svc_destroy(g_svc);
        g_svc = NULL;
    }
    g_svc_failed = 0;
    g_device = device;
    pthread_mutex_unlock(&g_mu);
    return g_fec_bound ? 0 : -1;
}

int pquic_fec_set_recover_mode(int mode) {
    if (mode != 0 && mode != 1) return -1;
    if (mode == 1 && (fecgpu_block_svc_rlc_decode_full == NULL || fecgpu_rlc_decode_host_full == NULL)) return -1;
    pthread_mutex_lock(&g_mu);
    g_recover_mode = mode;
    pthread_mutex_unlock(&g_mu);
    return 0;
}

int pquic_fec_get_recover_mode(void) {
    pthread_mutex_lock(&g_mu);
    const int mode = g_recover_mode;
    pthread_mutex_unlock(&g_mu);
    return mode;
}

uint64_t pquic_fec_singular_blocks(void) { return __atomic_load_n(&g_fec_singular_blocks, __ATOMIC_RELAXED); }

int pquic_fec_set_hooks_in_place(int on) {
    if (on != 0 && on != 1) return -1;
    if (on && (fecgpu_block_svc_rlc_encode_rows == NULL || fecgpu_block_svc_rlc_decode_rows == NULL ||
               fecgpu_block_svc_xor_encode_rows == NULL || fecgpu_block_svc_xor_decode_rows == NULL ||
               fecgpu_rlc_encode_rows_fused_host == NULL || fecgpu_rlc_decode_rows_fused_host == NULL ||
               fecgpu_rlc_decode_rows_fused_host_full == NULL || fecgpu_xor_encode_rows_host == NULL ||
               fecgpu_xor_decode_rows_host == NULL))
        return -1;
    pthread_mutex_lock(&g_mu);
    g_in_place = on;
    pthread_mutex_unlock(&g_mu);
    return 0;
}

int pquic_fec_get_hooks_in_place(void) {
    pthread_mutex_lock(&g_mu);
    const int on = g_in_place;
    pthread_mutex_unlock(&g_mu);
    return on;
}

int pquic_fec_register_heap(void *base, size_t bytes) {
    return base && bytes && fecgpu_host_register(base, bytes) == FECGPU_OK ? 0 : -1;
}

int pquic_fec_unregister_heap(void *base) { return base && fecgpu_host_unregister(base) == FECGPU_OK ? 0 : -1; }

void pquic_fec_hook_rows_stats(uint64_t out[4]) {
    pthread_mutex_lock(&g_mu);
    memcpy(out, g_row_stats, sizeof g_row_stats);
    pthread_mutex_unlock(&g_mu);
}

void pquic_fec_protoop_stats(pquic_fec_protoop_stats_t *out) {
    out->generate_calls = __atomic_load_n(&g_fec_stats.generate_calls, __ATOMIC_RELAXED);
    out->recover_calls = __atomic_load_n(&g_fec_stats.recover_calls, __ATOMIC_RELAXED);
    out->recovered_symbols = __atomic_load_n(&g_fec_stats.recovered_symbols, __ATOMIC_RELAXED);
    out->ref_ub_blocks = __atomic_load_n(&g_fec_stats.ref_ub_blocks, __ATOMIC_RELAXED);
    out->errors = __atomic_load_n(&g_fec_stats.errors, __ATOMIC_RELAXED);
    pthread_mutex_lock(&g_mu);
    out->svc_deadline_misses = g_svc ? fecgpu_block_svc_deadline_misses(g_svc) : 0;
    pthread_mutex_unlock(&g_mu);
}

int pquic_fec_layout(uint64_t out[8]) {
    out[0] = sizeof(pquic_fec_block_t);
    out[1] = sizeof(pquic_source_symbol_t);
    out[2] = sizeof(pquic_repair_symbol_t);
    out[3] = offsetof(pquic_fec_block_t, source_symbols);
    out[4] = offsetof(pquic_fec_block_t, repair_symbols);
    out[5] = offsetof(pquic_source_symbol_t, data);
    out[6] = offsetof(pquic_repair_symbol_t, data);
    out[7] = sizeof(pquic_repair_fpid_t);
    return 8;
}

static fecgpu_host_ctx_t *ctx(void) {
    if (!g_ctx) g_ctx = fecgpu_host_ctx_create(g_device, 1, 1u << 20);
    return g_ctx;
}

/* the worker ends within a poll of the quit flag; at exit it must not outlive the process's HIP state */
static void svc_atexit(void) {
    pthread_mutex_lock(&g_mu);
    fecgpu_block_svc_destroy(g_svc);
    g_svc = NULL;
    pthread_mutex_unlock(&g_mu);
}

static fecgpu_block_svc_t *svc(void) {
    static int at_exit;
    if (!g_svc && !g_svc_failed && !(g_svc = fecgpu_block_svc_create(g_device))) g_svc_failed = 1;
    if (g_svc && !at_exit) at_exit = !atexit(svc_atexit);
    return g_svc;
}

static int grow_pinned(uint8_t **p, size_t *cap, size_t need) {
    if (need <= *cap) return 0;
    size_t n = *cap ? *cap : 64 * 1024;
    while (n < need) n *= 2;
    uint8_t *q = fecgpu_host_alloc(n);
    if (!q) return -1;
    fecgpu_host_free(*p);
    *p = q;
    *cap = n;
    return 0;
}

static int stage(size_t src_bytes, size_t rep_bytes) {
    if (!g_aux && !(g_aux = fecgpu_host_alloc(sizeof *g_aux))) return -1;
    if (grow_pinned(&g_src, &g_src_cap, src_bytes) || grow_pinned(&g_rep, &g_rep_cap, rep_bytes ? rep_bytes : 4))
        return -1;
    return 0;
}

/* ------------------------------------------------------------------ create_fec_schemes */

/* create_rlc_fec_scheme_gf256.c:46-59: outputs [0] receiver scheme, [1] sender scheme
 * (the same object); returns 0 or PICOQUIC_ERROR_MEMORY.  The 64 KiB multiplication and
 * inverse tables of the reference are not needed: the device derives products from
 * GF(2^8) bit planes. */
protoop_arg_t pquic_fec_rlc_create_fec_schemes(picoquic_cnx_t *cnx) {
    if (!g_fec_bound) return PQUIC_FEC_ERR_UNBOUND;
    pquic_fec_scheme_t *fs = g_fec_api.my_malloc(cnx, sizeof *fs);
    if (!fs) return PQUIC_ERROR_MEMORY;
    fs->magic = RLC_MAGIC;
    fs->device = (uint32_t)g_device;
    g_fec_api.set_cnx(cnx, PQUIC_AK_CNX_OUTPUT, 0, (protoop_arg_t)(uintptr_t)fs);
    g_fec_api.set_cnx(cnx, PQUIC_AK_CNX_OUTPUT, 1, (protoop_arg_t)(uintptr_t)fs);
    return 0;
}

/* create_xor_fec_scheme.c:4-9: both outputs NULL */
protoop_arg_t pquic_fec_xor_create_fec_schemes(picoquic_cnx_t *cnx) {
    if (!g_fec_bound) return PQUIC_FEC_ERR_UNBOUND;
    g_fec_api.set_cnx(cnx, PQUIC_AK_CNX_OUTPUT, 0, 0);
    g_fec_api.set_cnx(cnx, PQUIC_AK_CNX_OUTPUT, 1, 0);
    return 0;
}

/* ------------------------------------------------------------------ in-place mode */

/* The row tables of one block (under g_mu).  A symbol whose data is 4-byte aligned and lies in page-locked
 * memory the engine knows is entered by its own address; any other goes through its row of g_src / g_rep
 * (stride L), which are page-locked. */
#define ROWS_MAX FECGPU_MAX_K /* a block's 100 symbols, a span's 128 columns and slots */
_Static_assert(ROWS_MAX >= PQUIC_FEC_MAX_SYMBOLS_PER_BLOCK && ROWS_MAX >= FECGPU_MAX_R, "row tables hold a span");
typedef struct {
    uint64_t src[ROWS_MAX], rep[ROWS_MAX];
    uint32_t src_len[ROWS_MAX], rep_len[ROWS_MAX];
    uint64_t src_dev, rep_dev; /* device addresses of g_src / g_rep */
    uint32_t L;
} rows_t;
static rows_t g_rows;

static int rows_begin(rows_t *t, int k, int r, uint32_t L) {
    if (stage((size_t)k * L, (size_t)r * L)) return -1;
    if (fecgpu_host_device_address(g_src, (size_t)k * L, &t->src_dev) != FECGPU_OK ||
        fecgpu_host_device_address(g_rep, (size_t)r * L, &t->rep_dev) != FECGPU_OK)
        return -1;
    t->L = L;
    return 0;
}

/* The address that stands for `n` bytes at `data`: their own when they can be used where they lie (1 into
 * *in_place), else that of staging row `stage_dev` (0). */
static uint64_t row_address(const void *data, uint32_t n, uint64_t stage_dev, int *in_place) {
    uint64_t d = 0;
    *in_place = n && !((uintptr_t)data & 3) && fecgpu_host_device_address(data, n, &d) == FECGPU_OK;
    g_row_stats[*in_place ? 0 : 1]++;
    return *in_place ? d : stage_dev;
}

/* an input row: n bytes of `data` (copied into its staging row unless they are used in place) */
static uint64_t row_input(const void *data, uint32_t n, uint8_t *stage_row, uint64_t stage_dev) {
    int in_place;
    if (!n) return 0; /* never dereferenced */
    const uint64_t a = row_address(data, n, stage_dev, &in_place);
    if (!in_place) memcpy(stage_row, data, n);
    return a;
}

static void row_call_done(int served) { g_row_stats[served ? 2 : 3]++; }

/* generate with the mode on (maxl > 0; under g_mu): the repairs are allocated first, in the order
 * fec_generate_finish allocates them, and the engine writes them where they lie */
static protoop_arg_t generate_in_place(picoquic_cnx_t *cnx, pquic_fec_block_t *fb, int xor_scheme, uint16_t maxl) {
    const int k = fb->total_source_symbols, r = fb->total_repair_symbols;
    const uint32_t fbn = fb->fec_block_number & 0xffffffu, blk = maxl, L = fec_pad4(maxl);
    rows_t *t = &g_rows;
    fecgpu_host_ctx_t *c = rows_begin(t, k, r, L) ? NULL : ctx();
    if (!c) {
        FEC_STAT_ADD(errors, 1);
        return PQUIC_FEC_ERR_UNBOUND;
    }
    pquic_repair_symbol_t *reps[PQUIC_FEC_MAX_SYMBOLS_PER_BLOCK];
    const int n = fec_generate_alloc(cnx, fb, maxl, reps);
    uint64_t copy[2] = {0, 0};
    int rc = 0;
    if (n) { /* the first n repairs do not depend on the later ones */
        for (int j = 0; j < k; j++) {
            const pquic_source_symbol_t *ss = fb->source_symbols[j];
            t->src_len[j] = ss ? ss->data_length : 0;
            t->src[j] = row_input(ss ? ss->data : NULL, t->src_len[j], g_src + (size_t)j * L, t->src_dev + (uint64_t)j * L);
        }
        for (int i = 0; i < n; i++) {
            int in_place;
            t->rep[i] = row_address(reps[i]->data, blk, t->rep_dev + (uint64_t)i * L, &in_place);
            if (!in_place) copy[i >> 6] |= 1ull << (i & 63);
        }
        fecgpu_block_svc_t *v = svc();
        if (!v)
            rc = FECGPU_ERR_INVALID;
        else if (xor_scheme)
            rc = fecgpu_block_svc_xor_encode_rows(v, t->src, t->src_len, t->rep[0], blk, (uint32_t)k);
        else
            rc = fecgpu_block_svc_rlc_encode_rows(v, t->src, t->src_len, t->rep, blk, (uint32_t)k, (uint32_t)n, fbn);
        const int served = rc == FECGPU_OK;
        if (rc == FECGPU_ERR_INVALID)
            rc = xor_scheme ? fecgpu_xor_encode_rows_host(c, t->src, t->src_len, t->rep, &blk, 1, (uint32_t)k, L)
                            : fecgpu_rlc_encode_rows_fused_host(c, t->src, t->src_len, t->rep, &blk, 1, (uint32_t)k,
                                                                (uint32_t)n, L, &fbn);
        if (!rc) row_call_done(served);
    }
    if (rc) {
        for (int i = 0; i < n; i++) {
            g_fec_api.my_free(cnx, reps[i]->data);
            g_fec_api.my_free(cnx, reps[i]);
        }
        FEC_STAT_ADD(errors, 1);
        return PQUIC_FEC_ERR_UNBOUND;
    }
    for (int i = 0; i < n; i++)
        if ((copy[i >> 6] >> (i & 63)) & 1) memcpy(reps[i]->data, g_rep + (size_t)i * L, maxl);
    return fec_generate_attach(fb, reps, n);
}

/* recover with the mode on (maxl > 0; under g_mu): the symbols a recovery would insert are allocated
 * first (fec_recover_alloc / _alloc_xor, as the batcher does) and the engine writes them where they lie */
static protoop_arg_t recover_in_place(picoquic_cnx_t *cnx, pquic_fec_block_t *fb, int xor_scheme, uint16_t maxl) {
    const int k = fb->total_source_symbols, r = xor_scheme ? 1 : fb->total_repair_symbols;
    const uint32_t blk = maxl, L = fec_pad4(maxl);
    rows_t *t = &g_rows;
    fecgpu_host_ctx_t *c = rows_begin(t, k, r, L) ? NULL : ctx();
    if (!c) {
        FEC_STAT_ADD(errors, 1);
        return PQUIC_FEC_ERR_UNBOUND;
    }
    pquic_source_symbol_t *pre[PQUIC_FEC_MAX_SYMBOLS_PER_BLOCK];
    if (xor_scheme) fec_recover_alloc_xor(cnx, fb, maxl, pre);
    else fec_recover_alloc(cnx, fb, maxl, pre);
    uint32_t seeds[PQUIC_FEC_MAX_SYMBOLS_PER_BLOCK];
    uint64_t sp[2] = {0, 0}, rp[2] = {0, 0}, copy[2] = {0, 0}, rec[2] = {0, 0};
    uint8_t st = FECGPU_BLOCK_NOTHING;
    for (int j = 0; j < k; j++) {
        const pquic_source_symbol_t *ss = fb->source_symbols[j];
        uint8_t *row = g_src + (size_t)j * L;
        const uint64_t row_dev = t->src_dev + (uint64_t)j * L;
        if (ss) { /* bytes past max_length are never read back (:205): truncate */
            t->src_len[j] = ss->data_length < maxl ? ss->data_length : maxl;
            t->src[j] = row_input(ss->data, t->src_len[j], row, row_dev);
            sp[j >> 6] |= 1ull << (j & 63);
            continue;
        }
        /* a missing source: the row its recovered bytes go to -- the symbol allocated for it, or its staging
         * row when that is not page-locked or was not allocated (fec_recover_finish_pre copies it out) */
        int in_place = 0;
        t->src_len[j] = 0;
        t->src[j] = pre[j] ? row_address(pre[j]->data, blk, row_dev, &in_place) : row_dev;
        if (!in_place) copy[j >> 6] |= 1ull << (j & 63);
    }
    for (int i = 0; i < r; i++) {
        const pquic_repair_symbol_t *rs = fb->repair_symbols[i];
        t->rep_len[i] = !rs ? 0 : rs->data_length < maxl ? rs->data_length : maxl;
        t->rep[i] = rs ? row_input(rs->data, t->rep_len[i], g_rep + (size_t)i * L, t->rep_dev + (uint64_t)i * L) : 0;
        if (rs) rp[i >> 6] |= 1ull << (i & 63);
        seeds[i] = rs ? rs->fpid.f.source_fpid.raw : 0; /* the repair's own FPID (:200), see fec_recover_stage */
    }
    const int full = !xor_scheme && g_recover_mode == 1;
    fecgpu_block_svc_t *v = svc();
    int rc;
    if (!v)
        rc = FECGPU_ERR_INVALID;
    else if (xor_scheme)
        rc = fecgpu_block_svc_xor_decode_rows(v, t->src, t->src_len, t->rep[0], blk, (uint32_t)k, sp, rp, &st, rec);
    else
        rc = fecgpu_block_svc_rlc_decode_rows(v, t->src, t->src_len, t->rep, t->rep_len, blk, (uint32_t)k, (uint32_t)r,
                                              seeds, sp, rp, full, &st, rec);
    const int served = rc == FECGPU_OK;
    if (rc == FECGPU_ERR_INVALID) {
        if (xor_scheme)
            rc = fecgpu_xor_decode_rows_host(c, t->src, t->src_len, t->rep, &blk, 1, (uint32_t)k, L, sp, rp, &st, rec);
        else if (full)
            rc = fecgpu_rlc_decode_rows_fused_host_full(c, t->src, t->src_len, t->rep, t->rep_len, &blk, 1, (uint32_t)k,
                                                        (uint32_t)r, L, seeds, sp, rp, &st, rec);
        else
            rc = fecgpu_rlc_decode_rows_fused_host(c, t->src, t->src_len, t->rep, t->rep_len, &blk, 1, (uint32_t)k,
                                                   (uint32_t)r, L, seeds, sp, rp, &st, rec);
    }
    if (rc) {
        for (int j = 0; j < k; j++)
            if (pre[j]) {
                g_fec_api.my_free(cnx, pre[j]->data);
                g_fec_api.my_free(cnx, pre[j]);
            }
        FEC_STAT_ADD(errors, 1);
        return PQUIC_FEC_ERR_UNBOUND;
    }
    row_call_done(served);
    uint64_t nrec = 0;
    const protoop_arg_t ret = xor_scheme ? fec_recover_finish_pre_xor(cnx, fb, st, rec, pre, copy, g_src, L, maxl, &nrec)
                                         : fec_recover_finish_pre(cnx, fb, st, rec, pre, copy, g_src, L, maxl, &nrec);
    if (nrec) FEC_STAT_ADD(recovered_symbols, nrec);
    return ret;
}

/* ------------------------------------------------------------------ generate */

static protoop_arg_t generate(picoquic_cnx_t *cnx, int xor_scheme) {
    if (!g_fec_bound) return PQUIC_FEC_ERR_UNBOUND;
    pquic_fec_block_t *fb = (pquic_fec_block_t *)(uintptr_t)g_fec_api.get_cnx(cnx, PQUIC_AK_CNX_INPUT, 0);
    uint16_t maxl = 0;
    const int chk = fec_generate_check(fb, xor_scheme, &maxl);
    if (chk == FEC_STAGE_REJECT) {
        FEC_STAT_ADD(errors, 1);
        return PQUIC_FEC_ERR_UNBOUND;
    }
    if (chk) return 1;
    const int k = fb->total_source_symbols, r = fb->total_repair_symbols;
    const uint32_t fbn = fb->fec_block_number & 0xffffffu;
    pthread_mutex_lock(&g_mu);
    FEC_STAT_ADD(generate_calls, 1);
    if (g_in_place && maxl) { /* (a block of empty symbols has no row to hand over: staged) */
        const protoop_arg_t ret = generate_in_place(cnx, fb, xor_scheme, maxl);
        pthread_mutex_unlock(&g_mu);
        return ret;
    }
    const uint32_t L = fec_pad4(maxl ? maxl : 1);
    int rc = stage((size_t)k * L, (size_t)r * L);
    fecgpu_host_ctx_t *c = rc ? NULL : ctx();
    if (c) {
        fec_generate_stage(fb, g_src, L);
        fecgpu_block_svc_t *v = xor_scheme ? NULL : svc();
        rc = v ? fecgpu_block_svc_rlc_encode(v, g_src, g_rep, (uint32_t)k, (uint32_t)r, L, fbn) : FECGPU_ERR_INVALID;
        if (rc == FECGPU_ERR_INVALID)
            rc = xor_scheme ? fecgpu_xor_encode_host(c, g_src, g_rep, 1, (uint32_t)k, L)
                            : fecgpu_rlc_encode_host(c, g_src, g_rep, 1, (uint32_t)k, (uint32_t)r, L, fbn, NULL);
    } else {
        rc = -1;
    }
    protoop_arg_t ret;
    if (rc) {
        FEC_STAT_ADD(errors, 1);
        ret = PQUIC_FEC_ERR_UNBOUND;
    } else {
        ret = fec_generate_finish(cnx, fb, g_rep, L, maxl);
    }
    pthread_mutex_unlock(&g_mu);
    return ret;
}

protoop_arg_t pquic_fec_rlc_generate_repair_symbols(picoquic_cnx_t *cnx) { return generate(cnx, 0); }
protoop_arg_t pquic_fec_xor_generate_repair_symbols(picoquic_cnx_t *cnx) { return generate(cnx, 1); }

/* ------------------------------------------------------------------ recover */

/* rlc_fec_scheme_gf256.c:134-251 and xor_fec_scheme.c:41-74.  The RLC equations are seeded by each
 * received repair's own FPID (:200), so blocks of the block framework ((fbn << 8) | i) and of the
 * sliding-window framework (block numbered by its window start, repairs (0 << 8) | i) both recover
 * as the reference does. */
static protoop_arg_t recover(picoquic_cnx_t *cnx, int xor_scheme) {
    if (!g_fec_bound) return PQUIC_FEC_ERR_UNBOUND;
    pquic_fec_block_t *fb = (pquic_fec_block_t *)(uintptr_t)g_fec_api.get_cnx(cnx, PQUIC_AK_CNX_INPUT, 0);
    uint16_t maxl = 0;
    const int chk = fec_recover_check(fb, xor_scheme, &maxl);
    if (chk == FEC_STAGE_REJECT) {
        FEC_STAT_ADD(errors, 1);
        return PQUIC_FEC_ERR_UNBOUND;
    }
    if (chk != FEC_STAGE_OK) return (protoop_arg_t)chk;
    const int k = fb->total_source_symbols, r = xor_scheme ? 1 : fb->total_repair_symbols;
    pthread_mutex_lock(&g_mu);
    FEC_STAT_ADD(recover_calls, 1);
    if (g_in_place && maxl) {
        const protoop_arg_t ret = recover_in_place(cnx, fb, xor_scheme, maxl);
        pthread_mutex_unlock(&g_mu);
        return ret;
    }
    const uint32_t L = fec_pad4(maxl ? maxl : 1);
    int rc = stage((size_t)k * L, (size_t)r * L);
    fecgpu_host_ctx_t *c = rc ? NULL : ctx();
    if (c) {
        aux_t *a = g_aux;
        a->st = FECGPU_BLOCK_NOTHING;
        a->rec[0] = a->rec[1] = 0;
        fec_recover_stage(fb, xor_scheme, maxl, g_src, g_rep, L, a->sp, a->rp, a->seeds);
        fecgpu_block_svc_t *v = xor_scheme ? NULL : svc();
        const int full = !xor_scheme && g_recover_mode == 1;  /* the mode of this call: read under g_mu */
        if (!v)
            rc = FECGPU_ERR_INVALID;
        else if (full)
            rc = fecgpu_block_svc_rlc_decode_full(v, g_src, g_rep, g_src, (uint32_t)k, (uint32_t)r, L, a->seeds, a->sp,
                                                  a->rp, &a->st, a->rec);
        else
            rc = fecgpu_block_svc_rlc_decode_seeded(v, g_src, g_rep, g_src, (uint32_t)k, (uint32_t)r, L, a->seeds,
                                                    a->sp, a->rp, &a->st, a->rec);
        if (rc == FECGPU_ERR_INVALID && full)
            rc = fecgpu_rlc_decode_host_full(c, g_src, g_rep, 1, (uint32_t)k, (uint32_t)r, L, 0, NULL, a->seeds, a->sp,
                                             a->rp, &a->st, a->rec);
        else if (rc == FECGPU_ERR_INVALID)
            rc = xor_scheme ? fecgpu_xor_decode_host(c, g_src, g_rep, 1, (uint32_t)k, L, a->sp, a->rp, &a->st, a->rec)
                            : fecgpu_rlc_decode_host_seeded(c, g_src, g_rep, 1, (uint32_t)k, (uint32_t)r, L, a->seeds,
                                                            a->sp, a->rp, &a->st, a->rec);
    } else {
        rc = -1;
    }
    protoop_arg_t ret;
    if (rc) {
        FEC_STAT_ADD(errors, 1);
        ret = PQUIC_FEC_ERR_UNBOUND;
    } else {
        ret = fec_recover_finish(cnx, fb, xor_scheme, g_aux->st, g_aux->rec, g_src, L, maxl, NULL);
    }
    pthread_mutex_unlock(&g_mu);
    return ret;
}

protoop_arg_t pquic_fec_rlc_recover(picoquic_cnx_t *cnx) { return recover(cnx, 0); }
protoop_arg_t pquic_fec_xor_recover(picoquic_cnx_t *cnx) { return recover(cnx, 1); }

/* ------------------------------------------------------------------ span recovery */

/* One span, blocking (pquic_fec_protoops.h): the checks and the pre-allocation of pquic_fec_batch_recover_span,
 * the row tables of recover_in_place -- whatever g_in_place says -- one span decode on rows, and the completion
 * of the batcher's span_finish. */
protoop_arg_t pquic_fec_rlc_recover_span(picoquic_cnx_t *cnx, const pquic_fec_span_t *sp,
                                         pquic_source_symbol_t **recovered, uint32_t *nrecovered) {
    if (nrecovered) *nrecovered = 0;
    if (!g_fec_bound || !sp || !recovered || !nrecovered) return PQUIC_FEC_ERR_UNBOUND;
    if (fecgpu_rlc_span_decode_rows_fused_host == NULL) return PQUIC_FEC_ERR_UNBOUND;
    if (sp->K < 1 || sp->K > FECGPU_MAX_K || sp->R < 1 || sp->R > FECGPU_MAX_R) return PQUIC_FEC_ERR_UNBOUND;
    if (!sp->src || !sp->rep || !sp->first_id || !sp->nss) return PQUIC_FEC_ERR_UNBOUND;
    const uint32_t K = sp->K, R = sp->R;
    uint16_t maxl = 0; /* the span's length: the longest repair */
    for (uint32_t i = 0; i < R; i++) {
        const pquic_repair_symbol_t *rs = sp->rep[i];
        const uint32_t off = sp->first_id[i] - sp->base_id; /* modulo 2^32 */
        const uint32_t n = rs ? rs->data_length : 0; /* 15 bits: no symbol is longer than 32767 bytes */
        if (!rs || (n && !rs->data)) return PQUIC_FEC_ERR_UNBOUND;
        if (!sp->nss[i] || off >= K || sp->nss[i] > K - off) return PQUIC_FEC_ERR_UNBOUND;
        if (n > maxl) maxl = (uint16_t)n;
    }
    uint32_t missing = 0;
    for (uint32_t x = 0; x < K; x++) {
        const pquic_source_symbol_t *ss = sp->src[x];
        const uint32_t n = ss ? ss->data_length : 0;
        if (!ss) missing++;
        else if (n && !ss->data) return PQUIC_FEC_ERR_UNBOUND;
    }
    for (uint32_t x = 0; x < K; x++) recovered[x] = NULL;
    if (!missing || !maxl) return 0; /* nothing to recover, or nothing to recover it from */
    const uint32_t blk = maxl, L = fec_pad4(maxl);
    pthread_mutex_lock(&g_mu);
    FEC_STAT_ADD(recover_calls, 1);
    rows_t *t = &g_rows;
    fecgpu_host_ctx_t *c = rows_begin(t, (int)K, (int)R, L) ? NULL : ctx();
    if (!c) {
        FEC_STAT_ADD(errors, 1);
        pthread_mutex_unlock(&g_mu);
        return PQUIC_FEC_ERR_UNBOUND;
    }
    pquic_source_symbol_t **pre = recovered; /* the symbols allocated for the missing columns, numbered by stream id */
    uint32_t seeds[ROWS_MAX];
    uint8_t roff[ROWS_MAX], rnss[ROWS_MAX];
    uint64_t spm[2] = {0, 0}, rpm[2] = {0, 0}, copy[2] = {0, 0}, rec[2] = {0, 0};
    uint8_t st = FECGPU_BLOCK_NOTHING;
    for (uint32_t x = 0; x < K; x++) {
        const pquic_source_symbol_t *ss = sp->src[x];
        uint8_t *row = g_src + (size_t)x * L;
        const uint64_t row_dev = t->src_dev + (uint64_t)x * L;
        if (ss) { /* a received source counts for at most the span's length */
            t->src_len[x] = ss->data_length < maxl ? ss->data_length : maxl;
            t->src[x] = row_input(ss->data, t->src_len[x], row, row_dev);
            spm[x >> 6] |= 1ull << (x & 63);
            continue;
        }
        /* a missing column: the row its recovered bytes go to -- the symbol allocated for it, or its staging row
         * when that is not page-locked or was not allocated (copied out below) */
        int in_place = 0;
        pre[x] = fec_new_source(cnx, sp->base_id + x, maxl);
        t->src_len[x] = 0;
        t->src[x] = pre[x] ? row_address(pre[x]->data, blk, row_dev, &in_place) : row_dev;
        if (!pre[x]) g_row_stats[1]++; /* its staging row, which row_address did not see */
        if (!in_place) copy[x >> 6] |= 1ull << (x & 63);
    }
    for (uint32_t i = 0; i < R; i++) {
        const pquic_repair_symbol_t *rs = sp->rep[i];
        t->rep_len[i] = rs->data_length; /* at most the span's length, which is the largest of them */
        t->rep[i] = row_input(rs->data, t->rep_len[i], g_rep + (size_t)i * L, t->rep_dev + (uint64_t)i * L);
        rpm[i >> 6] |= 1ull << (i & 63);
        seeds[i] = rs->fpid.f.source_fpid.raw; /* the repair's own FPID, as in fec_recover */
        roff[i] = (uint8_t)(sp->first_id[i] - sp->base_id);
        rnss[i] = sp->nss[i];
    }
    const int rc = fecgpu_rlc_span_decode_rows_fused_host(c, t->src, t->src_len, t->rep, t->rep_len, &blk, 1, K, R, L,
                                                          seeds, roff, rnss, spm, rpm, &st, rec);
    const int ok = !rc && st == FECGPU_BLOCK_RECOVERED;
    if (rc) FEC_STAT_ADD(errors, 1);
    else if (st == FECGPU_BLOCK_SINGULAR) __atomic_fetch_add(&g_fec_singular_blocks, 1, __ATOMIC_RELAXED);
    if (!rc) row_call_done(0);
    for (uint32_t x = 0; x < K; x++) { /* what the engine did not recover is freed first, in column order */
        if ((ok && ((rec[x >> 6] >> (x & 63)) & 1)) || !pre[x]) continue;
        g_fec_api.my_free(cnx, pre[x]->data);
        g_fec_api.my_free(cnx, pre[x]);
        pre[x] = NULL;
    }
    uint32_t nrec = 0;
    for (uint32_t x = 0; ok && x < K; x++) {
        if (!((rec[x >> 6] >> (x & 63)) & 1) || sp->src[x]) continue;
        const uint8_t *row = g_src + (size_t)x * L;
        if (!pre[x]) { /* the allocation before the call had failed: once more, skipped when that fails too */
            if (!(pre[x] = fec_new_source(cnx, sp->base_id + x, maxl))) continue;
            memcpy(pre[x]->data, row, maxl);
        } else if ((copy[x >> 6] >> (x & 63)) & 1) {
            memcpy(pre[x]->data, row, maxl);
        }
        nrec++;
    }
    if (nrec) FEC_STAT_ADD(recovered_symbols, nrec);
    pthread_mutex_unlock(&g_mu);
    *nrecovered = nrec;
    return rc ? PQUIC_FEC_ERR_UNBOUND : 0;
}

/* ---- source-symbol capture ---- */
static int skip_via_host(void *cnx, const uint8_t *bytes, size_t bytes_max, size_t *consumed, int *pure_ack) {
    return g_fec_api.skip_frame((picoquic_cnx_t *)cnx, (uint8_t *)bytes, bytes_max, consumed, pure_ack);
}

protoop_arg_t pquic_fec_packet_payload_to_source_symbol(picoquic_cnx_t *cnx) {
    if (!g_fec_bound || !g_fec_api.skip_frame) return PQUIC_FEC_ERR_UNBOUND;
    const uint8_t *payload = (const uint8_t *)g_fec_api.get_cnx(cnx, PQUIC_AK_CNX_INPUT, 0);
    uint8_t *buffer = (uint8_t *)g_fec_api.get_cnx(cnx, PQUIC_AK_CNX_INPUT, 1);
    const uint32_t length = (uint32_t)g_fec_api.get_cnx(cnx, PQUIC_AK_CNX_INPUT, 2);
    const uint64_t pn = (uint64_t)g_fec_api.get_cnx(cnx, PQUIC_AK_CNX_INPUT, 3);
    if (!buffer) return PQUIC_ERROR_MEMORY;                                /* :14-16 */
    return pquic_fec_payload_to_source_symbol(payload, length, pn, buffer, skip_via_host, cnx);
}
