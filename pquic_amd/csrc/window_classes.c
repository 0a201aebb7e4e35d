/*
 * pquic_amd/csrc/window_classes.c -- fecgpu_rlc_window_classes: the windows of a variable-length window
 * encode sorted into classes of one length (include/fecgpu.h).  Host C, no device call.
 */
#include "fecgpu.h"
#include "fecgpu_internal.h"

int fecgpu_rlc_window_classes(const uint8_t *wlen, uint64_t nwin, uint32_t kmax, uint32_t symbol_size, uint32_t *perm,
                              uint32_t *cls, uint32_t *nclasses, uint64_t *nchunks) {
    if (!wlen || !perm || !cls || !nclasses || !nchunks)
        return fecgpu_set_error_internal(FECGPU_ERR_INVALID, "window classes: NULL argument");
    if (kmax < 1 || kmax > FECGPU_MAX_K)
        return fecgpu_set_error_internal(FECGPU_ERR_INVALID, "window classes: kmax out of range [1,128]");
    if (symbol_size == 0 || (symbol_size & 3) || symbol_size > 65532)
        return fecgpu_set_error_internal(FECGPU_ERR_INVALID,
                                         "window classes: symbol_size must be a positive multiple of 4 (<= 65532)");
    if (nwin >= 0xffffffffull)
        return fecgpu_set_error_internal(FECGPU_ERR_INVALID, "window classes: 2^32 - 1 windows or more");
    uint64_t count[FECGPU_MAX_K + 1] = {0}, start[FECGPU_MAX_K + 1];
    for (uint64_t w = 0; w < nwin; w++) {
        if (wlen[w] < 1 || wlen[w] > kmax)
            return fecgpu_set_error_internal(FECGPU_ERR_INVALID, "window classes: wlen out of range [1,kmax]");
        count[wlen[w]]++;
    }
    /* the classes in order of length; class x: first[x], cnt[x], len[x], cchunk[x] at cls[x + {0,1,2,3} * kmax] */
    const uint64_t W = ((uint64_t)symbol_size + 15u) & ~(uint64_t)15;
    uint32_t *first = cls, *cnt = cls + kmax, *len = cls + 2 * (size_t)kmax, *cchunk = cls + 3 * (size_t)kmax;
    uint64_t pos = 0, chunk = 0;
    uint32_t nc = 0;
    for (uint32_t l = 1; l <= kmax; l++) {
        start[l] = pos;
        if (!count[l]) continue;
        if (chunk >= 0xffffffffull)
            return fecgpu_set_error_internal(FECGPU_ERR_INVALID, "window classes: 2^32 - 1 chunks or more");
        first[nc] = (uint32_t)pos;
        cnt[nc] = (uint32_t)count[l];
        len[nc] = l;
        cchunk[nc] = (uint32_t)chunk;
        nc++;
        pos += count[l];
        chunk += (count[l] * W + 2047) / 2048; /* the class's windows x bytes space in 2 KiB chunks of its own */
    }
    if (chunk >= 0xffffffffull)
        return fecgpu_set_error_internal(FECGPU_ERR_INVALID, "window classes: 2^32 - 1 chunks or more");
    for (uint32_t x = nc; x < kmax; x++) { /* no class: never the answer of the kernel's compare */
        first[x] = cnt[x] = len[x] = 0;
        cchunk[x] = 0xffffffffu;
    }
    /* stable: within a class the windows keep the caller's order */
    for (uint64_t w = 0; w < nwin; w++) perm[start[wlen[w]]++] = (uint32_t)w;
    *nclasses = nc;
    *nchunks = chunk;
    return FECGPU_OK;
}
