/*
 * tools/span_load.c -- host stand-in for a span receiver on the batching adapter
 * (pquic_fec_batch_recover_span, include/pquic_fec_batch.h) and on the blocking call
 * (pquic_fec_rlc_recover_span, include/pquic_fec_protoops.h), for the tests and the measurement.  Plays a
 * single-threaded picoquic receiver with several connections: every connection allocates from its own arena
 * (registered with the batcher or not), symbols are built from the caller's bytes, spans are submitted, and
 * every completion is recorded per ticket -- its place in the completion order, the value it returned and the
 * recovered columns with their bytes, lengths and FPIDs.  sl_run is the load leg: spans made of k / r / step
 * windows under independent loss, from several connections.
 */
#define _GNU_SOURCE  /* MAP_ANONYMOUS */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <time.h>

#include "fecgpu.h"
#include "pquic_fec_batch.h"

/* ---- the allocator: per connection, slots carved from one arena (picoquic/memory.c:72-95, 181-191), with a
 *      count of live allocations; symbol descriptors take small slots, symbol data 2112-byte ones; an exhausted
 *      arena falls back to the heap (tagged) ---- */
enum { BIG = 2112, SMALL = 64, HDR = 16 };
typedef union slot_u { union slot_u *next; uint8_t tag; } slot_u;
typedef struct {
    uint8_t *base;
    size_t bytes, used;
    slot_u *free_big, *free_small;
    long live;
    int registered;
} sl_arena_t;
struct st_picoquic_cnx_t { int id; sl_arena_t arena; };

static protoop_arg_t sl_get(picoquic_cnx_t *c, access_key_t ak, uint16_t p) { (void)c; (void)ak; (void)p; return 0; }
static void sl_set(picoquic_cnx_t *c, access_key_t ak, uint16_t p, protoop_arg_t v) { (void)c; (void)ak; (void)p; (void)v; }

static void *sl_malloc(picoquic_cnx_t *c, unsigned int n) {
    sl_arena_t *a = &c->arena;
    const int small = n <= SMALL - HDR;
    const size_t sz = small ? SMALL : BIG;
    slot_u **fl = small ? &a->free_small : &a->free_big, *s = *fl;
    if (n > BIG - HDR) s = NULL;
    else if (s) *fl = s->next;
    else if (a->base && a->used + sz <= a->bytes) {
        s = (slot_u *)(a->base + a->used);
        a->used += sz;
    }
    if (!s) {  /* heap: too large for a slot, or the arena is full */
        uint8_t *p = malloc((size_t)n + HDR);
        if (!p) return NULL;
        p[0] = 3;
        a->live++;
        return p + HDR;
    }
    s->tag = small ? 1 : 2;
    a->live++;
    return (uint8_t *)s + HDR;
}

static void sl_free(picoquic_cnx_t *c, void *p) {
    if (!p) return;
    sl_arena_t *a = &c->arena;
    slot_u *s = (slot_u *)((uint8_t *)p - HDR);
    a->live--;
    if (s->tag == 3) { free(s); return; }
    slot_u **fl = s->tag == 1 ? &a->free_small : &a->free_big;
    s->next = *fl;
    *fl = s;
}

static uint64_t now_us(void) {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (uint64_t)ts.tv_sec * 1000000u + (uint64_t)ts.tv_nsec / 1000u;
}

static uint64_t now_ns(void) {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (uint64_t)ts.tv_sec * 1000000000u + (uint64_t)ts.tv_nsec;
}

/* ---- the handle ---- */
typedef struct {
    int done;
    long order;
    uint64_t ret;
    uint32_t nrec, ncols;                 /* nrecovered as reported; columns found non-NULL in recovered[] */
    uint32_t *col, *fpid, *len;
    uint8_t **bytes;
    pquic_source_symbol_t **sym;          /* the symbols handed over, until sl_release */
    int conn;
    struct sl *h;
    /* the span as submitted: the caller's arrays copied, alive until the completion */
    pquic_fec_span_t sp;
    pquic_source_symbol_t **src;
    pquic_repair_symbol_t **rep;
    uint32_t *first_id;
    uint8_t *nss;
} ticket_t;

typedef struct sl {
    pquic_fec_batcher_t *b;
    picoquic_cnx_t *cnx;
    int nconn, device;
    void **syms;      /* symbols built by sl_source / sl_repair */
    int *sym_conn;
    long nsyms, syms_cap;
    ticket_t **tk;
    long ntk, tk_cap, completions;
} sl_t;

static const pquic_fec_host_api_t g_api = {sl_get, sl_set, sl_malloc, sl_free, NULL};

/* Opens a batcher and nconn connections with an arena of arena_bytes each; registered[c] != 0 registers
 * connection c's arena with the batcher.  Binds the host allocator (unbound again by sl_close). */
void *sl_open(int device, unsigned batch_blocks, unsigned max_delay_us, unsigned max_symbol, unsigned poll_blocks,
              int nconn, size_t arena_bytes, const uint8_t *registered) {
    sl_t *h = calloc(1, sizeof *h);
    if (!h || nconn < 1) { free(h); return NULL; }
    pquic_fec_bind_host(&g_api, device);
    const pquic_fec_batch_cfg_t cfg = {device, batch_blocks, max_delay_us, max_symbol, 2, poll_blocks};
    h->b = pquic_fec_batcher_create(&cfg);
    h->cnx = calloc((size_t)nconn, sizeof *h->cnx);
    if (!h->b || !h->cnx) goto fail;
    h->nconn = nconn;
    h->device = device;
    for (int c = 0; c < nconn; c++) {
        sl_arena_t *a = &h->cnx[c].arena;
        h->cnx[c].id = c;
        a->bytes = (arena_bytes + 4095) & ~(size_t)4095;
        void *p = mmap(NULL, a->bytes, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
        if (p == MAP_FAILED) goto fail;
        a->base = p;
        if (registered && registered[c]) {
            if (pquic_fec_batch_register_heap(h->b, a->base, a->bytes)) goto fail;
            a->registered = 1;
        }
    }
    return h;
fail:
    if (h->b) pquic_fec_batcher_destroy(h->b);
    for (int c = 0; h->cnx && c < nconn; c++)
        if (h->cnx[c].arena.base) munmap(h->cnx[c].arena.base, h->cnx[c].arena.bytes);
    free(h->cnx);
    free(h);
    pquic_fec_bind_host(NULL, device);
    return NULL;
}

static void ticket_free(ticket_t *t) {
    if (!t) return;
    for (uint32_t x = 0; x < t->ncols; x++) free(t->bytes[x]);
    free(t->col); free(t->fpid); free(t->len); free(t->bytes); free(t->sym);
    free(t->src); free(t->rep); free(t->first_id); free(t->nss);
    free(t);
}

void sl_close(void *hv) {
    sl_t *h = hv;
    if (!h) return;
    pquic_fec_batcher_destroy(h->b);  /* drains: every completion has run; unregisters the arenas */
    for (long i = 0; i < h->ntk; i++) ticket_free(h->tk[i]);
    for (int c = 0; c < h->nconn; c++) munmap(h->cnx[c].arena.base, h->cnx[c].arena.bytes);
    free(h->tk); free(h->syms); free(h->sym_conn); free(h->cnx);
    const int device = h->device;
    free(h);
    pquic_fec_bind_host(NULL, device);
}

/* live allocations of connection conn (conn < 0: of all) */
long sl_live(void *hv, int conn) {
    sl_t *h = hv;
    long n = 0;
    for (int c = 0; c < h->nconn; c++)
        if (conn < 0 || c == conn) n += h->cnx[c].arena.live;
    return n;
}

static long sym_add(sl_t *h, void *s, int conn) {
    if (h->nsyms == h->syms_cap) {
        const long nc = h->syms_cap ? 2 * h->syms_cap : 1024;
        void **ns = realloc(h->syms, sizeof *ns * (size_t)nc);
        if (!ns) return -1;
        h->syms = ns;
        int *ncn = realloc(h->sym_conn, sizeof *ncn * (size_t)nc);
        if (!ncn) return -1;
        h->sym_conn = ncn;
        h->syms_cap = nc;
    }
    h->syms[h->nsyms] = s;
    h->sym_conn[h->nsyms] = conn;
    return h->nsyms++;
}

/* A source symbol of connection conn holding len of the caller's bytes, FPID fpid; returns its id or -1. */
long sl_source(void *hv, int conn, const uint8_t *bytes, unsigned len, uint32_t fpid) {
    sl_t *h = hv;
    picoquic_cnx_t *c = &h->cnx[conn];
    pquic_source_symbol_t *s = sl_malloc(c, sizeof *s);
    uint8_t *d = sl_malloc(c, len ? len : 1);
    if (!s || !d) return -1;
    memset(s, 0, sizeof *s);
    if (len) memcpy(d, bytes, len);
    s->fpid.raw = fpid;
    s->data_length = (uint16_t)len;
    s->data = d;
    return sym_add(h, s, conn);
}

/* A repair symbol: seed_fpid its source FPID (the equation's seed), first_id its window start. */
long sl_repair(void *hv, int conn, const uint8_t *bytes, unsigned len, uint32_t seed_fpid, uint32_t first_id) {
    sl_t *h = hv;
    picoquic_cnx_t *c = &h->cnx[conn];
    pquic_repair_symbol_t *s = sl_malloc(c, sizeof *s);
    uint8_t *d = sl_malloc(c, len ? len : 1);
    if (!s || !d) return -1;
    memset(s, 0, sizeof *s);
    if (len) memcpy(d, bytes, len);
    s->fpid.f.source_fpid.raw = seed_fpid;
    s->fpid.f.fec_scheme_specific = first_id;
    s->data_length = (uint16_t)len;
    s->data = d;
    return sym_add(h, s, conn);
}

static void on_done(void *user, const pquic_fec_span_t *sp, pquic_source_symbol_t *const *rec, uint32_t nrec,
                    protoop_arg_t ret) {
    ticket_t *t = user;
    t->done++;
    t->order = t->h->completions++;
    t->ret = ret;
    t->nrec = nrec;
    uint32_t n = 0;
    for (uint32_t x = 0; x < sp->K; x++) n += rec[x] != NULL;
    t->ncols = n;
    if (!n) return;
    t->col = malloc(sizeof *t->col * n);
    t->fpid = malloc(sizeof *t->fpid * n);
    t->len = malloc(sizeof *t->len * n);
    t->bytes = calloc(n, sizeof *t->bytes);
    t->sym = malloc(sizeof *t->sym * n);
    n = 0;
    for (uint32_t x = 0; x < sp->K; x++) {
        if (!rec[x]) continue;
        t->col[n] = x;
        t->fpid[n] = rec[x]->fpid.raw;
        t->len[n] = rec[x]->data_length;
        t->bytes[n] = malloc(rec[x]->data_length ? rec[x]->data_length : 1);
        memcpy(t->bytes[n], rec[x]->data, rec[x]->data_length);
        t->sym[n] = rec[x];
        n++;
    }
}

/* A ticket for a span of connection conn as the caller describes it (sl_submit), with room in the handle. */
static ticket_t *ticket_new(sl_t *h, int conn, uint32_t base_id, uint32_t K, uint32_t R, const long *src_ids,
                            const long *rep_ids, const uint32_t *first_id, const uint8_t *nss, int fault) {
    ticket_t *t = calloc(1, sizeof *t);
    if (!t) return NULL;
    const uint32_t Ka = K ? K : 1, Ra = R ? R : 1;
    t->src = calloc(Ka > 256 ? 256 : Ka, sizeof *t->src);
    t->rep = calloc(Ra > 256 ? 256 : Ra, sizeof *t->rep);
    t->first_id = calloc(Ra > 256 ? 256 : Ra, sizeof *t->first_id);
    t->nss = calloc(Ra > 256 ? 256 : Ra, 1);
    if (!t->src || !t->rep || !t->first_id || !t->nss) { ticket_free(t); return NULL; }
    for (uint32_t x = 0; x < K && x < 256; x++) t->src[x] = src_ids[x] >= 0 ? h->syms[src_ids[x]] : NULL;
    for (uint32_t x = 0; x < R && x < 256; x++) {
        t->rep[x] = rep_ids[x] >= 0 ? h->syms[rep_ids[x]] : NULL;
        t->first_id[x] = first_id[x];
        t->nss[x] = nss[x];
    }
    t->sp = (pquic_fec_span_t){base_id, K, R, fault == 1 ? NULL : t->src, fault == 2 ? NULL : t->rep,
                               fault == 3 ? NULL : t->first_id, fault == 4 ? NULL : t->nss};
    t->h = h;
    t->conn = conn;
    if (h->ntk == h->tk_cap) {
        const long nc = h->tk_cap ? 2 * h->tk_cap : 256;
        ticket_t **nt = realloc(h->tk, sizeof *nt * (size_t)nc);
        if (!nt) { ticket_free(t); return NULL; }
        h->tk = nt;
        h->tk_cap = nc;
    }
    return t;
}

/* Submits a span of connection conn: src_ids[K] / rep_ids[R] are symbol ids (-1: NULL).  fault, for the
 * argument checks: 1 NULL src table, 2 NULL rep table, 3 NULL first_id, 4 NULL nss, 5 NULL done, 6 NULL span.
 * Returns the ticket (>= 0) when the call returned 0, -1 when it returned -1, -2 on a failure of its own. */
long sl_submit(void *hv, int conn, uint32_t base_id, uint32_t K, uint32_t R, const long *src_ids, const long *rep_ids,
               const uint32_t *first_id, const uint8_t *nss, uint64_t now, int fault) {
    sl_t *h = hv;
    ticket_t *t = ticket_new(h, conn, base_id, K, R, src_ids, rep_ids, first_id, nss, fault);
    if (!t) return -2;
    const int rc = pquic_fec_batch_recover_span(h->b, &h->cnx[conn], fault == 6 ? NULL : &t->sp, now,
                                                fault == 5 ? NULL : on_done, t);
    if (rc) {
        const int called = t->done;
        ticket_free(t);
        return called ? -3 : -1;  /* -3: refused, yet the callback ran */
    }
    h->tk[h->ntk] = t;
    return h->ntk++;
}

/* Runs a span of connection conn through the blocking call, pquic_fec_rlc_recover_span, and records what it
 * handed over as a completion: sl_submit's arguments; fault 1-4 and 6 as there, 7 NULL recovered[], 8 NULL
 * nrecovered.  Returns the ticket (>= 0) when the call returned 0, -1 when it returned PQUIC_FEC_ERR_UNBOUND
 * with *nrecovered == 0 and recovered[] untouched or NULL, -3 for any other outcome, -2 on a failure of its own. */
long sl_recover_span(void *hv, int conn, uint32_t base_id, uint32_t K, uint32_t R, const long *src_ids,
                     const long *rep_ids, const uint32_t *first_id, const uint8_t *nss, int fault) {
    sl_t *h = hv;
    ticket_t *t = ticket_new(h, conn, base_id, K, R, src_ids, rep_ids, first_id, nss, fault);
    if (!t) return -2;
    pquic_source_symbol_t *poison = (pquic_source_symbol_t *)(uintptr_t)1, *rec[256];
    for (int x = 0; x < 256; x++) rec[x] = poison;
    uint32_t nrec = 0xdead;
    const protoop_arg_t ret = pquic_fec_rlc_recover_span(&h->cnx[conn], fault == 6 ? NULL : &t->sp,
                                                         fault == 7 ? NULL : rec, fault == 8 ? NULL : &nrec);
    if (ret) {
        int clean = ret == PQUIC_FEC_ERR_UNBOUND && (fault == 8 || nrec == 0);
        for (int x = 0; x < 256; x++) clean = clean && (rec[x] == poison || rec[x] == NULL);
        ticket_free(t);
        return clean ? -1 : -3;
    }
    on_done(t, &t->sp, rec, nrec, ret);
    h->tk[h->ntk] = t;
    return h->ntk++;
}

int sl_poll(void *hv, uint64_t now) { return pquic_fec_batch_poll(((sl_t *)hv)->b, now); }
int sl_drain(void *hv) { return pquic_fec_batch_drain(((sl_t *)hv)->b); }

/* out: times the callback ran, completion order, ret, nrecovered, columns handed over */
void sl_ticket(void *hv, long ticket, int64_t out[5]) {
    const ticket_t *t = ((sl_t *)hv)->tk[ticket];
    out[0] = t->done; out[1] = t->order; out[2] = (int64_t)t->ret; out[3] = t->nrec; out[4] = t->ncols;
}

/* the recovered columns of a ticket: column, fpid.raw, data_length, and the bytes at stride `stride` */
void sl_ticket_cols(void *hv, long ticket, uint32_t *col, uint32_t *fpid, uint32_t *len, uint8_t *bytes, unsigned stride) {
    const ticket_t *t = ((sl_t *)hv)->tk[ticket];
    for (uint32_t x = 0; x < t->ncols; x++) {
        col[x] = t->col[x];
        fpid[x] = t->fpid[x];
        len[x] = t->len[x];
        memcpy(bytes + (size_t)x * stride, t->bytes[x], t->len[x] < stride ? t->len[x] : stride);
    }
}

/* frees the symbols a ticket's completion handed over, as the framework does once it has read them */
void sl_release(void *hv, long ticket) {
    sl_t *h = hv;
    ticket_t *t = h->tk[ticket];
    for (uint32_t x = 0; t->sym && x < t->ncols; x++) {
        sl_free(&h->cnx[t->conn], t->sym[x]->data);
        sl_free(&h->cnx[t->conn], t->sym[x]);
    }
    free(t->sym);
    t->sym = NULL;
}

/* the batcher's stats as u64 words; returns sizeof(pquic_fec_batch_stats_t) */
int sl_stats(void *hv, uint64_t *out, int nwords) {
    pquic_fec_batch_stats_t st;
    pquic_fec_batch_get_stats(((sl_t *)hv)->b, &st);
    memcpy(out, &st, (size_t)nwords * 8 < sizeof st ? (size_t)nwords * 8 : sizeof st);
    return (int)sizeof st;
}

/* sizeof the stats struct and the byte offsets of: submitted, completed, batches, immediate, engine_errors,
 * rows_in_place, rows_staged, deadline_holds, spans, span_symbols (no batcher needed) */
int sl_stats_layout(int out[10]) {
#define OFF(f) (int)__builtin_offsetof(pquic_fec_batch_stats_t, f)
    const int o[10] = {OFF(submitted), OFF(completed), OFF(batches), OFF(immediate), OFF(engine_errors),
                       OFF(rows_in_place), OFF(rows_staged), OFF(deadline_holds), OFF(spans), OFF(span_symbols)};
#undef OFF
    memcpy(out, o, sizeof o);
    return (int)sizeof(pquic_fec_batch_stats_t);
}

/* ---- the load leg ----
 * nconn connections with registered arenas (registered != 0), each holding `slots` spans of its stream: K =
 * (nwin - 1) * step + k columns under nwin windows of k symbols, r repairs each (R = nwin * r), L-byte symbols
 * coded once by the engine (window blocks: block number 0, so repair i of a window is seeded by i).  Every
 * submission redraws the span's losses -- each source and each repair lost independently with probability p --
 * and hands the received symbols over; a completion stamps the latency, counts and frees what was recovered.
 * nspans submissions in all, round-robin over the connections, polling as a receiver's event loop does.
 * out: [0] spans/s, [1] recovered symbols/s, [2] stream GiB/s (received bytes handed over), [3] p50 us, [4] p99
 * us, [5] lost source symbols, [6] recovered source symbols, [7] rows in place, [8] rows staged, [9] batches,
 * [10] engine errors, [11] wall s.  Returns 0, or -1. */
typedef struct {
    pquic_fec_span_t sp;
    pquic_source_symbol_t **all_src, **src;   /* [K] every source / the received ones */
    pquic_repair_symbol_t **all_rep, **rep;   /* [R] every repair / the received ones, compacted */
    uint32_t *first_id, *all_first;
    uint8_t *nss;
    uint64_t t_submit;
    picoquic_cnx_t *cnx;
    int busy;
    struct run *run;
} rslot_t;
struct run {
    uint64_t *lat;
    long nlat, recovered, lost;
};

static uint64_t rng_next(uint64_t *s) {
    uint64_t x = (*s += 0x9E3779B97F4A7C15ull);
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 27; x *= 0x94D049BB133111EBull; x ^= x >> 31;
    return x;
}

static void run_done(void *user, const pquic_fec_span_t *sp, pquic_source_symbol_t *const *rec, uint32_t nrec,
                     protoop_arg_t ret) {
    rslot_t *s = user;
    (void)ret;
    const uint64_t t = now_us();
    s->run->lat[s->run->nlat++] = t > s->t_submit ? t - s->t_submit : 0;
    s->run->recovered += nrec;
    for (uint32_t x = 0; x < sp->K; x++)
        if (rec[x]) { sl_free(s->cnx, rec[x]->data); sl_free(s->cnx, rec[x]); }
    s->busy = 0;
}

static int cmp_u64(const void *a, const void *b) {
    const uint64_t x = *(const uint64_t *)a, y = *(const uint64_t *)b;
    return (x > y) - (x < y);
}

/* The blocking call's latency: one connection (its arena registered or not) holds one span of nwin windows as
 * sl_run builds them; ncalls times its losses are redrawn and, when a source is lost and a repair arrived, the
 * received symbols go through pquic_fec_rlc_recover_span, timed from the call to its return; what it hands over
 * is freed outside the timed part.  out: [0] p50 us, [1] p99 us, [2] min us, [3] lost source symbols, [4] recovered source symbols, [5] rows
 * in place, [6] rows staged, [7] calls that returned an error, [8] calls timed.  Returns 0, or -1. */
int sl_run_blocking(int device, int k, int r, int step, int nwin, int L, double p, long ncalls, int registered,
                    unsigned seed, double *out) {
    const int K = (nwin - 1) * step + k, R = nwin * r;
    if (K < 1 || K > 128 || R < 1 || R > 128 || L < 4 || (L & 3) || L > BIG - HDR || ncalls < 1) return -1;
    int rc = -1;
    const uint8_t reg = registered ? 1 : 0;
    sl_t *h = sl_open(device, 64, 100, (unsigned)L, 0, 1, (size_t)(K + R) * (BIG + SMALL) * 4 + (1u << 20), &reg);
    if (!h) return -1;
    picoquic_cnx_t *cnx = &h->cnx[0];
    uint8_t *stream = fecgpu_host_alloc((size_t)K * L), *coded = fecgpu_host_alloc((size_t)R * L);
    uint32_t wrow[128], first_id[128], all_first[128];
    uint8_t nss[128];
    pquic_source_symbol_t *all_src[128], *src[128], *rec[128];
    pquic_repair_symbol_t *all_rep[128], *rep[128];
    fecgpu_host_ctx_t *ctx = fecgpu_host_ctx_create(device, 2, 1u << 22);
    uint64_t *lat = calloc((size_t)ncalls, sizeof *lat);
    if (!stream || !coded || !ctx || !lat) goto out;
    uint64_t g = seed * 2654435761u + 1;
    for (size_t i = 0; i < (size_t)K * L; i += 8) {
        const uint64_t v = rng_next(&g);
        memcpy(stream + i, &v, (size_t)K * L - i < 8 ? (size_t)K * L - i : 8);
    }
    for (int w = 0; w < nwin; w++) wrow[w] = (uint32_t)(w * step);
    if (fecgpu_rlc_window_encode_host(ctx, stream, (uint64_t)K, wrow, (uint64_t)nwin, (uint32_t)k, (uint32_t)r,
                                      (uint32_t)L, coded) != FECGPU_OK)
        goto out;
    const uint32_t base = 0xfffffff0u;  /* the ids wrap inside the span */
    for (int x = 0; x < K; x++) {
        const long id = sl_source(h, 0, stream + (size_t)x * L, (unsigned)L, base + (uint32_t)x);
        if (id < 0) goto out;
        all_src[x] = h->syms[id];
    }
    for (int x = 0; x < R; x++) {
        all_first[x] = base + (uint32_t)(x / r * step);
        const long id = sl_repair(h, 0, coded + (size_t)x * L, (unsigned)L, (uint32_t)(x % r), all_first[x]);
        if (id < 0) goto out;
        all_rep[x] = h->syms[id];
    }
    memset(nss, k, sizeof nss);
    const uint64_t thresh = p >= 1.0 ? UINT64_MAX : (uint64_t)(p * 18446744073709551615.0);
    long nlat = 0, lost = 0, recovered = 0, errors = 0;
    uint64_t rows0[4], rows1[4];
    pquic_fec_hook_rows_stats(rows0);
    for (long n = 0; n < ncalls; n++) {
        uint32_t nr = 0, nrec = 0;
        int gone_now = 0;
        for (int x = 0; x < K; x++) {
            const int gone = rng_next(&g) < thresh;
            src[x] = gone ? NULL : all_src[x];
            gone_now += gone;
        }
        if (!gone_now) continue;  /* nothing lost: the call would return before the engine */
        lost += gone_now;
        for (int x = 0; x < R; x++)
            if (rng_next(&g) >= thresh) {
                rep[nr] = all_rep[x];
                first_id[nr++] = all_first[x];
            }
        if (!nr) continue;  /* no repair arrived: nothing to call */
        const pquic_fec_span_t sp = {base, (uint32_t)K, nr, src, rep, first_id, nss};
        const uint64_t t0 = now_ns();
        const protoop_arg_t ret = pquic_fec_rlc_recover_span(cnx, &sp, rec, &nrec);
        lat[nlat++] = now_ns() - t0;
        if (ret) { errors++; continue; }
        recovered += nrec;
        for (int x = 0; x < K; x++)
            if (rec[x]) { sl_free(cnx, rec[x]->data); sl_free(cnx, rec[x]); }
    }
    pquic_fec_hook_rows_stats(rows1);
    qsort(lat, (size_t)nlat, sizeof *lat, cmp_u64);
    out[0] = nlat ? (double)lat[nlat / 2] * 1e-3 : 0;
    out[1] = nlat ? (double)lat[(long)((double)(nlat - 1) * 0.99)] * 1e-3 : 0;
    out[2] = nlat ? (double)lat[0] * 1e-3 : 0;
    out[3] = (double)lost;
    out[4] = (double)recovered;
    out[5] = (double)(rows1[0] - rows0[0]);
    out[6] = (double)(rows1[1] - rows0[1]);
    out[7] = (double)errors;
    out[8] = (double)nlat;
    rc = 0;
out:
    free(lat);
    if (ctx) fecgpu_host_ctx_destroy(ctx);
    fecgpu_host_free(stream);
    fecgpu_host_free(coded);
    sl_close(h);
    return rc;
}

int sl_run(int device, int nconn, int k, int r, int step, int nwin, int L, double p, long nspans, int slots,
           unsigned batch_blocks, unsigned max_delay_us, int registered, unsigned seed, double *out) {
    const int K = (nwin - 1) * step + k, R = nwin * r;
    if (K < 1 || K > 128 || R < 1 || R > 128 || L < 4 || (L & 3) || L > BIG - HDR || nconn < 1 || slots < 1) return -1;
    int rc = -1;
    uint8_t *reg = malloc((size_t)nconn);
    memset(reg, registered ? 1 : 0, (size_t)nconn);
    const size_t per_span = (size_t)(K + R) * (BIG + SMALL), arena = (size_t)slots * per_span * 2 + (1u << 20);
    sl_t *h = sl_open(device, batch_blocks, max_delay_us, (unsigned)L, 0, nconn, arena, reg);
    free(reg);
    if (!h) return -1;
    /* the payload: one stream of `slots` spans, coded once; every connection holds its own copy of the symbols */
    const long rows = (long)slots * K;
    uint8_t *stream = fecgpu_host_alloc((size_t)rows * L), *coded = fecgpu_host_alloc((size_t)slots * R * L);
    uint32_t *wrow = malloc(sizeof *wrow * (size_t)slots * nwin);
    fecgpu_host_ctx_t *ctx = fecgpu_host_ctx_create(device, 2, 1u << 22);
    rslot_t *rs = calloc((size_t)nconn * slots, sizeof *rs);
    struct run run = {calloc((size_t)nspans + 1, sizeof(uint64_t)), 0, 0, 0};
    if (!stream || !coded || !wrow || !ctx || !rs || !run.lat) goto out;
    uint64_t g = seed * 2654435761u + 1;
    for (size_t i = 0; i < (size_t)rows * L; i += 8) {
        const uint64_t v = rng_next(&g);
        memcpy(stream + i, &v, (size_t)rows * L - i < 8 ? (size_t)rows * L - i : 8);
    }
    for (int s = 0; s < slots; s++)
        for (int w = 0; w < nwin; w++) wrow[s * nwin + w] = (uint32_t)(s * K + w * step);
    /* windows (s, w) in order: repairs [s][w][r] = the span's slots in window order */
    if (fecgpu_rlc_window_encode_host(ctx, stream, (uint64_t)rows, wrow, (uint64_t)slots * nwin, (uint32_t)k,
                                      (uint32_t)r, (uint32_t)L, coded) != FECGPU_OK)
        goto out;
    for (int c = 0; c < nconn; c++)
        for (int s = 0; s < slots; s++) {
            rslot_t *q = &rs[c * slots + s];
            q->cnx = &h->cnx[c];
            q->run = &run;
            q->all_src = calloc((size_t)K, sizeof *q->all_src);
            q->src = calloc((size_t)K, sizeof *q->src);
            q->all_rep = calloc((size_t)R, sizeof *q->all_rep);
            q->rep = calloc((size_t)R, sizeof *q->rep);
            q->first_id = calloc((size_t)R, sizeof *q->first_id);
            q->all_first = calloc((size_t)R, sizeof *q->all_first);
            q->nss = malloc((size_t)R);
            if (!q->all_src || !q->src || !q->all_rep || !q->rep || !q->first_id || !q->all_first || !q->nss) goto out;
            const uint32_t base = (uint32_t)(c * 1000003 + s * K);
            for (int x = 0; x < K; x++) {
                const long id = sl_source(h, c, stream + ((size_t)s * K + x) * L, (unsigned)L, base + (uint32_t)x);
                if (id < 0) goto out;
                q->all_src[x] = h->syms[id];
            }
            for (int w = 0; w < nwin; w++)
                for (int i = 0; i < r; i++) {
                    const int x = w * r + i;
                    const long id = sl_repair(h, c, coded + ((size_t)s * R + x) * L, (unsigned)L, (uint32_t)i,
                                              base + (uint32_t)(w * step));
                    if (id < 0) goto out;
                    q->all_rep[x] = h->syms[id];
                    q->all_first[x] = base + (uint32_t)(w * step);
                }
            memset(q->nss, k, (size_t)R);
            q->sp = (pquic_fec_span_t){base, (uint32_t)K, 0, q->src, q->rep, q->first_id, q->nss};
        }
    const uint64_t thresh = p >= 1.0 ? UINT64_MAX : (uint64_t)(p * 18446744073709551615.0);
    uint64_t bytes = 0;
    long submitted = 0;
    int next = 0;
    pquic_fec_batch_stats_t st0, st1;
    pquic_fec_batch_get_stats(h->b, &st0);
    const uint64_t t0 = now_us();
    while (submitted < nspans) {
        rslot_t *q = &rs[next];
        next = (next + 1) % (nconn * slots);
        while (q->busy) pquic_fec_batch_poll(h->b, now_us());
        uint32_t nr = 0;
        for (int x = 0; x < K; x++) {
            const int lost = rng_next(&g) < thresh;
            q->src[x] = lost ? NULL : q->all_src[x];
            run.lost += lost;
            bytes += lost ? 0 : (uint64_t)L;
        }
        for (int x = 0; x < R; x++)
            if (rng_next(&g) >= thresh) {
                q->rep[nr] = q->all_rep[x];
                q->first_id[nr++] = q->all_first[x];
                bytes += (uint64_t)L;
            }
        submitted++;
        if (!nr) continue;  /* no repair arrived: nothing to submit */
        q->sp.R = nr;
        q->busy = 1;
        q->t_submit = now_us();
        if (pquic_fec_batch_recover_span(h->b, q->cnx, &q->sp, q->t_submit, run_done, q)) goto out;
        if ((submitted & 15) == 0) pquic_fec_batch_poll(h->b, now_us());
    }
    pquic_fec_batch_drain(h->b);
    const double wall = (double)(now_us() - t0) * 1e-6;
    pquic_fec_batch_get_stats(h->b, &st1);
    qsort(run.lat, (size_t)run.nlat, sizeof *run.lat, cmp_u64);
    out[0] = (double)nspans / wall;
    out[1] = (double)run.recovered / wall;
    out[2] = (double)bytes / wall / (double)(1u << 30);
    out[3] = run.nlat ? (double)run.lat[run.nlat / 2] : 0;
    out[4] = run.nlat ? (double)run.lat[(long)((double)(run.nlat - 1) * 0.99)] : 0;
    out[5] = (double)run.lost;
    out[6] = (double)run.recovered;
    out[7] = (double)(st1.rows_in_place - st0.rows_in_place);
    out[8] = (double)(st1.rows_staged - st0.rows_staged);
    out[9] = (double)(st1.batches - st0.batches);
    out[10] = (double)(st1.engine_errors - st0.engine_errors);
    out[11] = wall;
    rc = 0;
out:
    if (h->b) pquic_fec_batch_drain(h->b);
    for (int i = 0; rs && i < nconn * slots; i++) {
        free(rs[i].all_src); free(rs[i].src); free(rs[i].all_rep); free(rs[i].rep);
        free(rs[i].first_id); free(rs[i].all_first); free(rs[i].nss);
    }
    free(rs);
    free(run.lat);
    free(wrow);
    if (ctx) fecgpu_host_ctx_destroy(ctx);
    fecgpu_host_free(stream);
    fecgpu_host_free(coded);
    sl_close(h);
    return rc;
}
