/*
 * pquic_amd/csrc/span_layout.c -- fecgpu_rlc_span_layout: from the windows of a receiver's repairs to the
 * span the span decode solves (include/fecgpu.h).  Host C, no device call.
 */
#include "fecgpu.h"
#include "fecgpu_internal.h"

int fecgpu_rlc_span_layout(const uint32_t *first_id, const uint8_t *nss, uint32_t m, uint32_t *base_id, uint32_t *K,
                           uint8_t *off) {
    if (m == 0) return fecgpu_set_error_internal(FECGPU_ERR_INVALID, "span layout: no repair");
    if (!first_id || !nss || !base_id || !K || !off)
        return fecgpu_set_error_internal(FECGPU_ERR_INVALID, "span layout: NULL argument");
    /* window starts relative to the first repair's, modulo 2^32: ids on both sides of a wrap stay neighbours */
    int64_t lo = 0, hi = 0;
    for (uint32_t i = 0; i < m; i++) {
        const int64_t d = (int32_t)(first_id[i] - first_id[0]);
        if (d < lo) lo = d;
        if (d + nss[i] > hi) hi = d + nss[i];
    }
    if (hi == lo) return fecgpu_set_error_internal(FECGPU_ERR_INVALID, "span layout: every window is empty");
    if (hi - lo > FECGPU_MAX_K)
        return fecgpu_set_error_internal(FECGPU_ERR_INVALID, "span layout: the windows span more than 128 symbols");
    *base_id = first_id[0] + (uint32_t)lo;
    *K = (uint32_t)(hi - lo);
    for (uint32_t i = 0; i < m; i++) off[i] = (uint8_t)((int64_t)(int32_t)(first_id[i] - first_id[0]) - lo);
    return FECGPU_OK;
}
