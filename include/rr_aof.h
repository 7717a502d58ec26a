/*
 * rr_aof.h — flat batch -> AOF rewrite commands on the GPU (the AOF half).
 *
 * Under `aof-use-rdb-preamble no` the rewrite child walks every db (rewriteAppendOnlyFileRio,
 * aof.c:1302-1389).  For an evicted value (shared.valueInRock, :1330) it fetches the blob, builds a robj
 * with desObject, uses it once to print RESP commands (:1342-1370, aof.c:921-1135) and frees it.  These
 * calls print those commands straight from the flat form of rr_format.h, so the child builds no object.
 *
 * For value i, out->data[offsets[i] .. offsets[i+1]) holds the commands rewriteAppendOnlyFileRio writes
 * for the key keys[i] holding the object desObject builds from value i, followed by its PEXPIREAT when
 * it has an expiry.  Concatenated in order behind rr_aof_select's bytes the slices are one db's section
 * of the rewritten file.
 *
 * Primitives (rio.c:406-445)
 *   rioWriteBulkCount(prefix, n)   prefix | ll2string(n) | CRLF
 *   rioWriteBulkString(s, len)     "$" len CRLF | bytes | CRLF; len 0 gives "$0\r\n\r\n"
 *   rioWriteBulkLongLong(v)        the bulk string of ll2string(v)
 *   rioWriteBulkDouble(d)          the bulk string of snprintf("%.17g", d).  For every non-NaN double
 *                                  that text is rr_d2string's (rr_d2string.h): d2string's branches for
 *                                  infinity and zero print what %.17g prints ("inf", "-inf", "0", "-0"),
 *                                  and its integer shortcut (|v| < 2^52, integral) prints at most 16
 *                                  digits, which %.17g prints the same way: no exponent below 10^17 and
 *                                  no fraction.  tests/test_aof.py holds the two against each other.
 *   the key                        always a bulk string (initStaticStringObject, aof.c:1337; :926-927)
 *
 * Per type
 *   STRING          "*3\r\n$3\r\nSET\r\n" | key | value (aof.c:1342-1348).  RAW / EMBSTR: the bulk string
 *                   of the STR descriptor; INT: rioWriteBulkLongLong of the INT descriptor (:924-925)
 *   aggregates      a command holds at most RR_AOF_ITEMS_PER_CMD = 64 items (AOF_REWRITE_ITEMS_PER_CMD,
 *                   aof.c:945, :978, :1037, :1118).  With c = min(64, items left) each command is
 *                   "*" (2 + c) CRLF (List, Set) or "*" (2 + 2c) CRLF (ZSet, Hash), the verb as a bulk
 *                   string, the key, then the c items.  An aggregate with no items writes no command.
 *   LIST_QUICKLIST  RPUSH (aof.c:935-965); an item is one descriptor: INT as its decimal
 *                   (entry.longval), STR as a bulk string.  A STR that the quicklist keeps as an integer
 *                   entry prints the same bytes: string2ll takes only what ll2string prints.
 *   SET_INTSET      SADD (:972-988); an item is one INT descriptor, as its decimal
 *   SET_HT          SADD (:989-1007); an item is one STR descriptor.  Exactly the members
 *                   rr_rdbsave_batch writes: the value's n_elems descriptors
 *   HASH_HT         HMSET (:1111-1135); an item is field, value: two STR descriptors
 *   ZSET_SKIPLIST   ZADD (:1054-1076); an item is STR member, SCORE: written score first
 *                   (rioWriteBulkDouble), then the member
 *   HASH_ZIPLIST    HMSET; the items are the entry descriptors behind the ZLRAW, two an item; an INT
 *                   entry is written as its decimal (:1095-1099), a STR entry as a bulk string
 *   ZSET_ZIPLIST    ZADD (:1019-1053); the entry descriptors behind the ZLRAW are member, score, ...;
 *                   written score first.  The score is %.17g of zzlGetScore (t_zset.c:721-741):
 *                     an INT entry    (double) v: round to nearest, ties to even, then printed.
 *                                     2^53 + 1 gives "9007199254740992", INT64_MAX "9.2233720368547758e+18"
 *                     a STR entry     strtod of its text, done in exact integer arithmetic
 *                                     (csrc/rr_strtod_impl.h, one text for host and device).  Taken:
 *                                       "inf", "-inf", and
 *                                       -? ( digits+ [ . digits* ] | . digits+ ) ( [eE] [+-]? digits+ )?
 *                                     of at most 40 bytes and at most 17 significant digits, counted
 *                                     from the first non-zero digit through the last non-zero one.
 *                                     Overflow prints "inf" / "-inf", underflow "0" / "-0", subnormals
 *                                     are exact.  Every text rr_d2string prints for a non-NaN double is
 *                                     taken and prints itself, so every ziplist the reference built
 *                                     itself is converted.  Every other text — "nan", hex, a leading
 *                                     "+" or space, "infinity", "INF", 18 significant digits or more,
 *                                     41 bytes or more, garbage — gives the VALUE the status
 *                                     RR_AOF_E_CPU: the reference's strtod takes some prefix of it,
 *                                     which the CPU path prints.  No sub-range of the grammar above is
 *                                     left out.
 *
 * Expiry (aof.c:1365-1370): when expires != NULL and expires[i] != -1 the value's commands are followed
 * by "*3\r\n$9\r\nPEXPIREAT\r\n" | key | rioWriteBulkLongLong(expires[i]); after an empty aggregate too.
 *
 * Deviations
 *   - SET_HT, HASH_HT and ZSET_SKIPLIST are written in the flat form's order, as rr_rdbsave.h has it:
 *     the reference walks dictNext under a per-process random hash seed; any order loads the same object.
 *   - A ZSET_ZIPLIST with no entries writes no command (and its PEXPIREAT, if any); the reference asserts
 *     there (aof.c:1028) and never holds one.
 *   - A NaN SCORE descriptor gives RR_AOF_E_CPU (%.17g prints "nan" or "-nan" by the sign; the decoder
 *     never produces one: RR_E_NAN).
 *
 * Status, in this order of precedence; every value with a non-zero status has size 0, writes nothing
 * and counts in rr_totals.n_bad:
 *   RR_E_ENCODE       rr_encode_batch's rule (rr_serdes.h, tests/encode_expect.py): status != 0 on entry,
 *                     descriptors or payload outside the caller's buffers, kinds that do not fit the
 *                     type.  For a ziplist value that rule looks at the ZLRAW only; here the entry
 *                     descriptors behind it must be an even number of STR (inside the arena) or INT
 *   RR_RDBFILE_E_KEY  the key slice is reversed, past keys->data_cap, or 2^31 - 16 bytes or more
 *   RR_AOF_E_CPU      a ziplist value that holds only its ZLRAW descriptor (a RR_CTX_ZL_RAW batch) and
 *                     is not the 11-byte empty ziplist; a score text that is not taken; a NaN SCORE
 *   RR_E_CAPACITY     the value would end past out->data_cap (its size still counts in the offsets)
 * offsets[0..n] are complete whatever data_cap is.  Nothing outside [elems, elems + elem_cap),
 * [arena, arena + arena_cap) and [keys->data, keys->data + keys->data_cap) is read.  Offsets are 64-bit.
 * rr_totals: n_elems the sum of every value's n_elems field, bytes = offsets[n], n_bad as above, payload
 * the STR bytes written as bulk strings by the values written (score texts and keys are not counted).
 */
#ifndef RR_AOF_H
#define RR_AOF_H

#include "rr_serdes.h"
#include "rr_rdbfile.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RR_AOF_ITEMS_PER_CMD 64      /* AOF_REWRITE_ITEMS_PER_CMD, server.h */
#define RR_AOF_E_CPU         56      /* left to the CPU path: see "Status" above */
#define RR_AOF_MAX_WAVES     16384u  /* a wave a value; a launch has at most this many, a grid stride beyond */
#define RR_AOF_SCORE_TEXT_MAX 40     /* the longest score text taken */

/* Upper bound on the bytes of a batch of n values with n_elems descriptors whose STR lengths sum to
 * payload_bytes and whose key lengths sum to key_bytes:
 *     128 n + 32 n_elems + payload_bytes + key_bytes * (2 + n_elems / 64), rounded up to 16.
 *   per descriptor  "$" + at most 10 digits + CRLF + body + CRLF: 15 + len for a string; a decimal or a
 *                   score text is at most 24 bytes: 30
 *   per command     "*" + at most 10 digits + CRLF, the verb (at most "$5\r\nHMSET\r\n", 11 bytes) and the
 *                   key's bulk string (at most 15 + len): 39 + key.  A value of m descriptors writes at
 *                   most 1 + m / 64 commands and one PEXPIREAT ("*3\r\n$9\r\nPEXPIREAT\r\n", 19 bytes, the
 *                   key's bulk string, and at most 27 bytes of time): 100 + 31 m + key * (2 + m / 64)
 * The key is repeated in every command, so the sums alone cannot bound it better than by the product:
 * one value may own every descriptor and every key byte.  A caller with many values does better with a
 * call at data_cap 0 first: offsets[n] is then the exact size. */
uint64_t rr_aof_bound(uint64_t n, uint64_t n_elems, uint64_t payload_bytes, uint64_t key_bytes);

/* Host: "*2\r\n$6\r\nSELECT\r\n$<digits>\r\n<dbi>\r\n" (aof.c:1310-1318) into buf; returns its length, or 0
 * when cap is too small (32 bytes always do) or dbi is negative. */
int rr_aof_select(uint8_t *buf, uint64_t cap, int dbi);

/* Host: the text rioWriteBulkDouble prints for the score zzlGetScore reads from a ziplist string entry
 * text[0, len), into buf (at most RR_D2STRING_MAX = 24 bytes, no NUL); returns its length, or -1 for a
 * text that is not taken ("ZSET_ZIPLIST" above).  The device runs the same statements. */
int rr_aof_score_text(char *buf, const char *text, uint64_t len);

/* Device-resident: every pointer on ctx's device.  out->n == keys->n == in->n; out->data 16-byte aligned;
 * keys->data[keys->offsets[i] .. keys->offsets[i+1]) is value i's key; expires (ms, -1 none) may be NULL:
 * no value has an expiry.  Writes out->offsets[0..n], out->data, status[0..n) and *d_totals.  Three
 * launches on `stream` (sizes, scan, emit), a wave a value, no host synchronisation; scratch comes from
 * the context (rr_ctx_reserve or a warm call before a graph capture, as for every call). */
int rr_aof_batch(rr_ctx *ctx, const rr_flat_batch *in, const rr_blob_batch *keys, const int64_t *expires,
                 rr_blob_batch *out, uint8_t *status, rr_totals *d_totals, void *stream);

/* The same over host pointers, staged through the context's device buffers; blocks.  key_bytes is
 * keys->data_cap; data receives min(offsets[n], data_cap) bytes. */
int rr_aof_batch_host(rr_ctx *ctx, const rr_value *values, const rr_elem *elems, uint64_t n_elems,
                      const uint8_t *arena, uint64_t arena_bytes, uint64_t n, const uint8_t *key_data,
                      const uint64_t *key_offsets, uint64_t key_bytes, const int64_t *expires, uint8_t *data, uint64_t data_cap,
                      uint64_t *offsets, uint8_t *status, rr_totals *totals);

#ifdef __cplusplus
}
#endif
#endif
