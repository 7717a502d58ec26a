/*
 * rock_serdes_compat.h — RedRock's legacy serdes entry points (src/rock_serdes.h:47-55) on the
 * engine, for a build inside a Redis tree.
 *
 * The bodies are redrock_old_amd/compat/rock_serdes_compat.c.  They need Redis's robj / sds /
 * dict / quicklist / intset / skiplist (server.h), so this header declares them only when
 * compiled inside a RedRock tree: -DRR_REDIS_TREE, after #include "server.h".
 *
 *   desObject / desString   one blob: the engine's host codec (rr_host.h) on the calling thread
 *                           (the GPU path's exact verdicts and flat form), then the robj;
 *   serObject               one robj: described in place and written by the host codec into a
 *                           fresh zmalloc'd sds;
 *   the batch forms         below the measured crossover the same host codec per value, at or
 *                           above it the GPU (rr_decode_batch_host / rr_encode_batch_host);
 *   any nonzero per-value status, and any engine error, ends in serverPanic() — the
 *   reference aborts through serverAssert/serverPanic on the same inputs (rock_serdes.c).
 *
 * So rock.c and rock_hotkey.c link against these unchanged: the per-key calls cost what the
 * reference's own C costs, and no call of theirs waits on a GPU launch.  A fork child (BGSAVE /
 * AOF rewrite, rock.c:527-550) always takes the host codec and never touches the HIP runtime.
 * INTEGRATION.md shows the wiring.
 */
#ifndef ROCK_SERDES_COMPAT_H
#define ROCK_SERDES_COMPAT_H

#include "rr_serdes.h"
#include "rr_rdb.h"

#ifdef RR_REDIS_TREE
/* rock_serdes.h:47 declares 2 args; the definition (rock_serdes.c:133) takes the lru too, and
 * that is the one provided (nothing outside rock_serdes.c calls it). */
robj *desString(char *s, size_t len, uint32_t lru);
sds serObject(robj *o);                 /* rock_serdes.h:48, rock_serdes.c:512 */
robj *desObject(void *buf, size_t len); /* rock_serdes.h:49, rock_serdes.c:538 */

/* Batch forms: n blobs -> n robj (out[i] == desObject(bufs[i], lens[i])), n robj -> n sds
 * (out[i] == serObject(objs[i])): the host codec per value below the crossover, one GPU call at
 * or above it (rr_compat_set_route). */
void rr_compat_des_batch(void *const *bufs, const size_t *lens, size_t n, robj **out);
void rr_compat_ser_batch(robj *const *objs, size_t n, sds *out);

/* Row f4 (rr_rdb.h): the fork child's batch restore.  k keys of database dbid, held in the
 * parent's RocksDB snapshot, requested over the child's pipes (rock_rdb.c:240-267) in one FLAT
 * request: the parent's service (rr_rdb_serve) decodes them on its GPU and the robj are built
 * here from the records — out[i] == loadValFromRockForRdb(dbid, keys[i]) (rock.c:527-550).
 * The child never touches the GPU. */
void rr_compat_rdb_load_batch(int fd_req, int fd_resp, int dbid, sds *keys, size_t k, robj **out);

/* GPU the calling thread's engine context is created on (default 0; set before first use). */
void rr_compat_set_device(int device);

/* rock_serdes.h:51-55: the debug round trips of `ROCK testserdes*` (rock.c:170-184), over the
 * engine, logging through serverLog as the reference's do (rock_serdes.c:626-901). */
void _test_ser_des_string(void);
void _test_ser_des_list(void);
void _test_ser_des_set(void);
void _test_ser_des_hash(void);
void _test_ser_des_zset(void);

/* Routing of desObject / serObject and the batch forms: AUTO (the default) = the host codec
 * below the measured crossover (values per call: RR_COMPAT_GPU_MIN_SER, default 16384, for the
 * encode; RR_COMPAT_GPU_MIN_DES, default 0 = never, for the decode; environment), the GPU at or
 * above it; HOST / GPU force one route (tests, benches).  A fork child (rock.c:527-550) never takes the
 * GPU route: under AUTO or HOST it decodes on its own CPU, under GPU the engine panics rather than
 * touch the parent's HIP runtime. */
#define RR_COMPAT_ROUTE_AUTO 0
#define RR_COMPAT_ROUTE_HOST 1
#define RR_COMPAT_ROUTE_GPU  2
void rr_compat_set_route(int route);

/* The ziplist check.  Strict (the compiled-in default): desObject and the batch forms walk every
 * Hash / ZSet ziplist and panic on one whose entries, zltail, zllen or pair count do not parse —
 * stricter than the reference, which checks only that the stored byte count equals the rest of the
 * blob and copies the ziplist blind (rock_serdes.c:356-366, :455-466).  Off: exactly the
 * reference's test, in O(1) — desObject accepts what the reference accepts at the reference's
 * cost, and the batch forms give the same objects on the host and the GPU route
 * (RR_CTX_ZL_RAW, rr_serdes.h).  The environment's RR_COMPAT_ZL_CHECK (1 = strict, 0 = off) sets
 * the default, read at the first call; this call overrides it.  rr_compat_rdb_load_batch applies
 * the calling process's check to the records the parent's service decoded: strict here, a ziplist
 * that arrives as its ZLRAW alone (a parent in raw mode) is walked here and a corrupt one panics;
 * off here, the parent sets RR_CTX_ZL_RAW on the context it gives rr_rdb_serve — a ziplist its
 * strict walk rejected carries no bytes to rebuild it from, and that pairing panics by name. */
void rr_compat_set_ziplist_check(int strict);

/* Process exit: every GPU call through this shim is counted in flight; the owner's exit waits
 * (at most 10 s) for the count to drain, and a thread calling in after the exit began parks
 * rather than enter the HIP runtime being torn down (RedRock's rock thread, rock.c:615, is never
 * joined).  A thread's engine context is destroyed when the thread ends.  Tests:
 * rr_compat_in_flight = the GPU calls in flight; rr_compat_test_hold_teardown(ms) makes the next
 * thread-exit context teardown sleep `ms` inside the count (rr_compat_test_holding says it
 * started); rr_compat_test_as_child(1) routes this process as a fork child would. */
int rr_compat_in_flight(void);
void rr_compat_test_hold_teardown(int ms);
int rr_compat_test_holding(void);
void rr_compat_test_as_child(int on);
#endif

#endif
