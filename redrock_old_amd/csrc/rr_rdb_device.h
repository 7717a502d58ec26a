// rr_rdb_device.h — the RDB wire format's lengths and integers, shared by the RDB kernels
// (rr_rdbsave.hip, rr_rdbload.hip, rr_rdbconvert.hip, rr_rdbfile.hip).  Line references are to the reference's rdb.c.
#pragma once
#include "rr_device.h"

namespace rr {

// ---- rdbSaveLen (rdb.c:147-178) ----
__device__ __forceinline__ uint32_t len_bytes(uint64_t len) {
    return len < 64 ? 1u : len < 16384 ? 2u : len <= 0xFFFFFFFFull ? 5u : 9u;
}
// nb <= 8 bytes of v, by one lane.  Unrolled into eight predicated stores: a loop over a lane's own
// byte count is one more level of divergent control flow, and each level holds an exec mask in an
// SGPR pair.
__device__ __forceinline__ void put_be(uint8_t *d, uint64_t v, uint32_t nb) {
#pragma unroll
    for (uint32_t k = 0; k < 8; ++k)
        if (k < nb) d[k] = (uint8_t)(v >> (8 * (nb - 1 - k)));
}
__device__ __forceinline__ void put_le(uint8_t *d, uint64_t v, uint32_t nb) {
#pragma unroll
    for (uint32_t k = 0; k < 8; ++k)
        if (k < nb) d[k] = (uint8_t)(v >> (8 * k));
}
__device__ __forceinline__ uint32_t put_len(uint8_t *d, uint64_t len) {
    if (len < 64) { d[0] = (uint8_t)len; return 1; }
    if (len < 16384) { d[0] = (uint8_t)(0x40 | (len >> 8)); d[1] = (uint8_t)len; return 2; }
    if (len <= 0xFFFFFFFFull) { d[0] = 0x80; put_be(d + 1, len, 4); return 5; }
    d[0] = 0x81;
    put_be(d + 1, len, 8);
    return 9;
}
// ---- rdbEncodeInteger (rdb.c:241-261) ----
__device__ __forceinline__ bool is_i32(int64_t v) { return v >= -2147483648ll && v <= 2147483647ll; }
__device__ __forceinline__ uint32_t rint_bytes(int64_t v) { return v >= -128 && v <= 127 ? 2u : v >= -32768 && v <= 32767 ? 3u : 5u; }
__device__ __forceinline__ void put_rint(uint8_t *d, int64_t v) {
    const uint32_t nb = rint_bytes(v) - 1;
    d[0] = (uint8_t)(0xC0 | (nb == 1 ? 0 : nb == 2 ? 1 : 2));
    put_le(d + 1, (uint64_t)v, nb);
}
// rdbSaveRawString's integer branch (rdb.c:416-422, rdbTryIntegerEncoding :307-321): up to 11 bytes
// that are the canonical decimal (what ll2string gives back: string2ll's strict form) of an int32
__device__ __forceinline__ bool raw_is_int(const uint8_t *s, uint32_t len, int64_t &v) {
    return len <= 11 && zip_try_int(s, len, v) && is_i32(v);
}
// ---- ziplist entries (ziplist.c:332-364, :480-534): an integer entry's data bytes and encoding byte, a
// string entry's header bytes ----
__device__ __forceinline__ uint32_t zint_bytes(int64_t v) {
    return v >= 0 && v <= 12 ? 0u : v >= -128 && v <= 127 ? 1u : v >= -32768 && v <= 32767 ? 2u
         : v >= -8388608 && v <= 8388607 ? 3u : is_i32(v) ? 4u : 8u;
}
__device__ __forceinline__ uint32_t zint_enc(int64_t v) {
    const uint32_t nb = zint_bytes(v);
    return nb == 0 ? 0xF1u + (uint32_t)v : nb == 1 ? 0xFEu : nb == 2 ? 0xC0u : nb == 3 ? 0xF0u : nb == 4 ? 0xD0u : 0xE0u;
}
__device__ __forceinline__ uint32_t zstr_hdr(uint32_t len) { return len <= 0x3F ? 1u : len <= 0x3FFF ? 2u : 5u; }

}  // namespace rr
