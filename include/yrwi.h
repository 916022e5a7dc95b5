/* yrwi.h -- C ABI of libyrwi, the MI355X-native YaCy RWI query engine.
 *
 * Drop-in boundary for YaCy's reverse-word-index query hot path.  Each entry
 * point names the Java interface it replaces (paths relative to
 * /root/reference/source/net/yacy).  INTEGRATION.md shows the JNI / Panama
 * binding a YaCy maintainer would add.
 *
 * Conventions:
 *   - int return codes: 0 = OK, < 0 = error (YRWI_E_*); message via yrwi_last_error();
 *   - "no result" is an empty result (n = 0), never an error -- as in
 *     ReferenceContainer.joinExcludeContainers (ReferenceContainer.java:318,322);
 *   - the caller owns every host buffer; the library owns device memory;
 *   - a context is bound to one GPU and is not thread-safe: one context per
 *     host thread, or serialise calls;
 *   - rows are YaCy's 40-byte WordReferenceRow layout (WordReferenceRow.java:49-72),
 *     i.e. the bytes of RowSet.chunkcache (RowCollection.java:68).
 */
#ifndef YRWI_H
#define YRWI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define YRWI_ROW_BYTES 40
#define YRWI_HASH_BYTES 12
#define YRWI_MAX_TERMS 8          /* include or exclude terms per query */
#define YRWI_MAX_K 3000           /* WeakPriorityBlockingQueue bound, SearchEvent.java:118 */
#define YRWI_MAX_DISTANCE_ANY 2147483647 /* Integer.MAX_VALUE: unquoted query, yacysearch.java:643 */

enum {
  YRWI_OK = 0,
  YRWI_E_ARG = -1,           /* bad argument / capacity too small */
  YRWI_E_HASH = -2,          /* url or term hash not well-formed Base64 (Base64Order.java:96-106) */
  YRWI_E_UNSORTED = -3,      /* rows not strictly ascending by url hash (and sorted != 0) */
  YRWI_E_HIP = -4,           /* HIP runtime error */
  YRWI_E_NOMEM = -5,         /* device allocation failed (SpaceExceededException) */
  YRWI_E_RCCL = -6,          /* collective failed */
  YRWI_E_NULL_LANGUAGE = -7, /* language cell is 0x0000: the reference throws NPE in
                                ASCII.getBytes(null) (WordReferenceVars.java:315, ReferenceOrder.java:260) */
  YRWI_E_UNSUPPORTED = -8,
  YRWI_E_LIMIT = -9,         /* list longer than 53,687,091 rows (RowSet.java:90-92) */
  YRWI_E_CAPACITY = -10,     /* search event tables full (max_postings given to yrwi_event_open too small) */
  YRWI_E_IO = -11            /* file could not be created, written or renamed */
};

typedef struct yrwi_ctx yrwi_ctx;

/* RankingProfile public int coefficients, in the declaration order of
 * RankingProfile.java:81-88.  Defaults: yrwi_profile_default(). */
typedef struct yrwi_profile {
  int32_t coeff_domlength, coeff_date, coeff_wordsintitle, coeff_wordsintext, coeff_phrasesintext,
      coeff_llocal, coeff_lother, coeff_urllength, coeff_urlcomps, coeff_hitcount,
      coeff_posintext, coeff_posofphrase, coeff_posinphrase, coeff_authority, coeff_worddistance,
      coeff_appurl, coeff_app_dc_title, coeff_app_dc_creator, coeff_app_dc_subject,
      coeff_app_dc_description, coeff_appemph, coeff_catindexof, coeff_cathasimage,
      coeff_cathasaudio, coeff_cathasvideo, coeff_cathasapp, coeff_urlcompintoplist,
      coeff_descrcompintoplist, coeff_prefer, coeff_termfrequency, coeff_language, coeff_citation;
} yrwi_profile;

/* One ranked result: a ReverseElement of SearchEvent.rwiStack
 * (WeakPriorityBlockingQueue.java:400-426). */
typedef struct yrwi_hit {
  uint8_t urlhash[12];
  int32_t tiebreak; /* ByteArray.hashCode(urlhash) (ByteArray.java:80-84) */
  int64_t score;    /* ReferenceOrder.cardinal(WordReference) (ReferenceOrder.java:223-265) */
} yrwi_hit;

/* Per-query constraints that SearchEvent.addRWIs applies before a posting enters
 * rwiStack (SearchEvent.java:736-806), and the doubledom pull order of
 * pullOneRWI(skipDoubleDom) (:1297-1394).  Normalisation still covers the whole
 * joined container; these only decide which postings are ranked. */
typedef struct yrwi_filter {
  uint8_t constraint[4];        /* QueryParams.constraint as Bitfield bytes (bit j: byte j>>3, bit j&7) */
  int32_t has_constraint;       /* constraint != null; testFlags :2459-2474 */
  int32_t all_of_constraint;    /* QueryParams.allofconstraint */
  int32_t contentdom;           /* ContentDomain code: -1 ALL, 0 TEXT, 1 IMAGE, 2 AUDIO, 3 VIDEO, 4 APP */
  int32_t strict_contentdom;    /* QueryParams.isStrictContentDom(): test the doctype, not the flags */
  char language[8];             /* QueryModifier.language, NUL terminated; "" = any */
  uint8_t sitehash[6];          /* QueryModifier.sitehash: host hash = url-hash chars 6..11 */
  uint8_t alt_sitehash[6];      /* DigestURL.hosthash of the www./non-www. variant (:716-718) */
  int32_t has_sitehash, has_alt_sitehash;
  const uint8_t* siteexcludes;  /* nsiteexcludes * 6 bytes (QueryParams.siteexcludes); used without sitehash */
  int32_t nsiteexcludes;
  const uint8_t* urlhashes;     /* nurlhashes * 12 bytes already in SearchEvent.urlhashes (doublecheck) */
  int32_t nurlhashes;
  int32_t skip_double_dom;      /* results in pullOneRWI(true) order: new hosts first (stack bound 3000) */
  int32_t* flagcount;           /* out: SearchEvent.flagcount[32] over the postings past the doublecheck, or NULL */
} yrwi_filter;

/* A query: QueryGoal include/exclude word hashes (QueryGoal.java:229-240) plus
 * QueryParams.maxDistance, the ranking profile and the target language. */
typedef struct yrwi_query_desc {
  const uint8_t* incl;        /* nincl * 12 bytes (word hashes) */
  int32_t nincl;
  const uint8_t* excl;        /* nexcl * 12 bytes */
  int32_t nexcl;
  int32_t max_distance;       /* YRWI_MAX_DISTANCE_ANY or #terms-1 for quoted queries */
  int32_t k;                  /* results wanted (<= YRWI_MAX_K) */
  const yrwi_profile* profile;
  char language[8];           /* ReferenceOrder.language, NUL terminated (any length) */
  int64_t now_ms;             /* System.currentTimeMillis() of the request; 0 = now */
  const yrwi_filter* filter;  /* NULL: unconstrained query */
  /* TermSearch's urlselection (TermSearch.java:42-62 -> AbstractIndex.searchConjunction :96-128):
   * nurlselection url hashes (12 bytes each; NULL / 0: none).  Every include and exclude
   * container is restricted to these urls before the conjunction, as
   * ReferenceContainerCache.get(key, urlselection) does (ReferenceContainerCache.java:448-470):
   * J1, the J2 fold order and every J3 dispatch then see the restricted sizes.  (IndexCell.get,
   * YaCy's segment index, ignores the argument (IndexCell.java:353-386) and the local search
   * passes null (SearchEvent.java:619).)  A selection with two or more include terms runs as a
   * chained fold: more than four include terms, or a maxDistance filter (quoted query), with a
   * selection: YRWI_E_UNSUPPORTED. */
  const uint8_t* urlselection;
  int32_t nurlselection;
} yrwi_query_desc;

typedef struct yrwi_stats {
  int64_t postings_in;   /* sum of include + exclude list lengths */
  int64_t joined;        /* rows of the joined container (before exclusion) */
  int64_t bytes_alg;     /* algorithmic bytes B = sum K + 12 sum n_excl + 23 t m_out */
  int64_t bytes_join;    /* sum K over the merge-path join jobs (the k_join launches timed in t_join_ns), K as the
                            reference dispatches the step (J3) */
  int64_t t_join_ns;     /* device time of the k_join launches (HIP events on the context stream) */
  int64_t t_norm_ns, t_score_ns, t_total_ns;
  int32_t n_join_launches, n_enum_steps, n_test_steps;
  int32_t n_realloc;     /* device-wide allocation events (scratch or pinned staging growth) during the call */
  int64_t bytes_probe;   /* sum K over the probe-executed join jobs (timed in t_probe_ns), K as the reference
                            dispatches the step (J3) */
  int64_t t_probe_ns;    /* device time of the k_probe launches */
  int64_t bytes_compact; /* bytes k_compact moves: per joined row 12 B pair + url id read, the 32-B ranking
                            record of the accumulated side and 16 B of the joined side's (by-test steps: one
                            32-B record) read, 32-B record + url id written */
  int64_t t_compact_ns;  /* device time of the compaction launches (k_compact and / or k_compact_sum, which also
                            writes the normalisation pieces of the queries that need no other pass) */
  int64_t t_kernels_ns;  /* device time of all the batch's kernel launches (HIP events around every group of
                            back-to-back launches; host waits and collectives excluded) */
  /* SURVEY.md §8(d) bytes with no step credited for reads its kernel never makes: every join step
     (merge, probe, exclusion) is charged min(K, the bytes its kernel loads) -- merge tiles: 4-B url ids
     of both sides; url-id bitmap probe: the smaller side's 4-B ids + one 16-B bitmap word per id;
     range probe: the ids + the larger list's range or a 128-B leaf line per id, whichever is less.
     bytes_probe_loaded / _capped: the probe-executed include steps (k_probe); bytes_join_capped: the
     merge-executed include steps (k_join); bytes_alg_capped: the whole path (joins, exclusions and
     23 t m_out) */
  int64_t bytes_probe_loaded;
  int64_t bytes_probe_capped;
  int64_t bytes_features;    /* 23 t m_out: the ranking-feature bytes of the joined containers (k_compact's share) */
  int64_t bytes_join_capped;
  int64_t bytes_alg_capped;
  /* every k_probe dispatch of the call, include and exclusion steps alike (rocprofv3 counts them all):
     their number and device time (HIP events around each) */
  int64_t n_probe_dispatches;
  int64_t t_probe_all_ns;
  /* rank phase, per pass: the k_reduce launch (with k_piece_merge, which merges the compaction's pieces)
     and the k_score launches (k_shard_fin / k_score_full excluded: the populations rocprofv3 averages),
     HIP events around each; the bytes their kernels must read: k_reduce the 32-B ranking record of every
     joined row of the queries without pieces (+ its 1-B exclusion mark), k_score the same records of
     every query (an upper bound: chunks pruned by the per-query threshold read only words 2-3) */
  int64_t n_rank_passes;
  int64_t t_reduce_ns;
  int64_t t_scorek_ns;
  int64_t bytes_reduce;
  int64_t bytes_score;
  /* chained folds: the k_chain launches, their device time (HIP events around k_chain alone, the
     population rocprofv3 averages) and their SURVEY.md §8(d) bytes -- the later fold steps' K and the
     exclusions' 12 n_e, each charged min(K, the bytes k_chain loads for it) */
  int64_t n_chain_launches;
  int64_t t_chain_ns;
  int64_t bytes_chain;
  /* identical queries of one pass of a batch part run once (YRWI_SHARE=0: every query
     runs): the queries that took an earlier identical query's result, their share of postings_in and
     of joined.  postings_in and joined keep their per-query meaning (a repeat counts its lists and its
     representative's rows); every byte, launch and time field counts executed work only. */
  int64_t queries_shared;
  int64_t postings_shared;
  int64_t joined_shared;
} yrwi_stats;

/* ---- profile helpers (RankingProfile.java) ---- */
void yrwi_profile_default(yrwi_profile* p);                 /* RankingProfile(TEXT) :90-125 */
void yrwi_profile_all_zero(yrwi_profile* p);                /* allZero() :200-233 */
int yrwi_profile_parse(const char* prefix, const char* ext, yrwi_profile* out); /* :127-189 */

/* ---- context ---- */
int yrwi_open(int device, yrwi_ctx** out);
/* One shard of a URL-hash-range partitioned index (Distribution.java:153-158):
 * rank r of `world` (power of two) owns url hashes whose first character index
 * c satisfies c >> (6 - log2(world)) == r.  `nccl_id` is the 128-byte
 * ncclUniqueId from yrwi_get_unique_id() on rank 0, broadcast by the caller.
 * The shards merge their partial results over RCCL (Protocol.java:802 merges
 * peers' results).  The ranks of a node first post their devices' PCI bus ids
 * in the node's host mailbox: ranks that share one device (RCCL refuses a
 * duplicate GPU) run the device collectives host-staged through shared memory
 * instead, as does an id starting with "YRWI-HOSTSTAGE".  Ranks on distinct
 * devices use RCCL only: if ncclCommInitRank fails the call returns YRWI_E_RCCL
 * and yrwi_last_error(NULL) gives RCCL's error string.  yrwi_shard_info says
 * which transport a context runs on. */
int yrwi_open_shard(int device, int rank, int world, const uint8_t nccl_id[128], yrwi_ctx** out);
int yrwi_get_unique_id(uint8_t nccl_id[128]);
void yrwi_close(yrwi_ctx* ctx);
/* ctx's last error; NULL: why the calling thread's last yrwi_open / yrwi_open_shard failed */
const char* yrwi_last_error(yrwi_ctx* ctx);

enum {
  YRWI_TRANSPORT_NONE = 0,        /* not sharded (yrwi_open) */
  YRWI_TRANSPORT_RCCL = 1,        /* RCCL communicators (xGMI between the node's GPUs) */
  YRWI_TRANSPORT_HOSTSTAGED = 2,  /* ranks share one device: host shared memory (/dev/shm) */
  YRWI_TRANSPORT_LOOPBACK = 3     /* in-process test group */
};
typedef struct yrwi_transport_info {
  int32_t transport;       /* YRWI_TRANSPORT_* */
  int32_t rank, world;
  int32_t rccl_ranks;      /* ncclCommCount of lane 0's communicator (0: no communicator) */
  int32_t lanes;           /* lanes (batches in flight) */
  int32_t lanes_own_comm;  /* lanes with a communicator of their own (ncclCommSplit) */
  int32_t device_peers;    /* other ranks of the group on this rank's device (-1: not exchanged) */
  int32_t mailbox;         /* 1: list sizes summed through the node's host mailbox */
  char pci_bus_id[16];     /* this rank's device */
} yrwi_transport_info;
/* The transport of a (shard) context and its communicator's rank count:
 * Distribution.java:153-158 partitions, Protocol.java:802 merges over it. */
int yrwi_shard_info(yrwi_ctx* ctx, yrwi_transport_info* out);

/* ---- index (IndexCell.add / RowSet import; the lists are what
 *      Index.get(termHash) returns, IndexCell.java:353-386) ---- */
/* Stores (or replaces) the posting list of `term`.  rows40: n rows of 40 bytes.
 * sorted != 0 promises ascending unique url hashes (validated); sorted == 0
 * sorts (duplicate url hashes: the first occurrence wins, RowSet.mergeEnum). */
int yrwi_put_list(yrwi_ctx* ctx, const uint8_t term[12], const uint8_t* rows40, int64_t n, int sorted);
int yrwi_list_size(yrwi_ctx* ctx, const uint8_t term[12], int64_t* n);
/* Index.get(termHash) for callers off the query path (AbstractIndex.java:116,
 * IndexCell.java:353-386; e.g. TermSearch.inclusion() for the index abstracts,
 * SearchEvent.java:513-531): the 40-byte rows of `term`'s list on this context
 * (its url-hash shard when sharded), ascending by url hash.  *n = the list size
 * (0: no list); YRWI_E_ARG when cap < *n (nothing copied). */
int yrwi_get_list(yrwi_ctx* ctx, const uint8_t term[12], uint8_t* rows40, int64_t cap, int64_t* n);
/* ---- index updates on the device (yrwi_update.hip): the caller keeps no host copy of a
 *      list and sends only the change.  Both calls wait for the batches in flight, as
 *      yrwi_put_list does, and take the rows they are given: a sharded context does not
 *      filter them to its url-hash range (the caller sends each shard its own). ---- */
enum {
  YRWI_ADD_REPLACE = 0, /* RowSet.put, what IndexCell.add(termHash, entry) does: the last candidate stays */
  YRWI_ADD_KEEP = 1,    /* RowSet.mergeEnum, the heap loader's rule: the first candidate stays */
  YRWI_ADD_RECENT = 2   /* ReferenceContainer.putAllRecent: a later candidate takes the place unless its
                           lastModified (column a, bytes 12-13) is strictly smaller */
};
typedef struct yrwi_update_stats {
  int64_t terms;          /* lists created, changed or emptied by the call */
  int64_t new_terms, emptied_terms;
  int64_t added;          /* batch postings whose url was new to their list */
  int64_t replaced;       /* batch postings that took the place of an existing row */
  int64_t dropped;        /* batch postings that lost (to an existing row or another batch row) */
  int64_t removed;        /* postings removed (yrwi_remove_postings) */
  int32_t launches;       /* kernel launches, device-library calls, copies and memsets the call enqueued:
                             a function of the batch's bytes, never of the number of terms touched */
  int32_t syncs;          /* host waits on the device the call made (staging growth on a lane's first
                             large batch not counted); independent of the terms touched */
} yrwi_update_stats;
/* IndexCell.add in bulk: posting i is rows40 + 40 i, for the list of term terms12 + 12 i, in any
 * order.  For each (term, url hash) the candidates are the list's row, if it has one, and then the
 * batch's rows of that pair in batch order; `policy` says which one stays.  Lists stay strictly
 * ascending by url hash; a term without a list gets one.  added + replaced + dropped == n.  Atomic:
 * on YRWI_E_HASH (term or url hash), YRWI_E_NULL_LANGUAGE, YRWI_E_LIMIT (a list would pass
 * 53,687,091 rows) or YRWI_E_NOMEM nothing has changed.  st may be NULL. */
int yrwi_add_postings(yrwi_ctx* ctx, const uint8_t* terms12, const uint8_t* rows40, int64_t n, int policy,
                      yrwi_update_stats* st);
/* IndexCell.remove(termHash, urlHashes) for each of nterms terms; nterms == 0: every list of the
 * context (Segment.removeAllUrlReferences without the document's words).  Duplicate urls and terms
 * count once, unknown terms and absent urls are ignored; a list left empty disappears as after
 * yrwi_put_list(n = 0).  st->removed = rows removed.  st may be NULL. */
int yrwi_remove_postings(yrwi_ctx* ctx, const uint8_t* terms12, int32_t nterms, const uint8_t* urls12,
                         int64_t nurls, yrwi_update_stats* st);
/* Removes every posting whose url hash carries one of the nhosts host hashes (hosts6 + 6 i: url-hash
 * characters 6..11, as yrwi_filter.sitehash) from the named lists; nterms == 0: from every list.
 * It behaves exactly as yrwi_remove_postings(ctx, terms12, nterms, U, |U|, st) with U = the url hashes
 * in the selected lists whose characters 6..11 are in the host set: duplicate hosts and terms count
 * once, unknown terms and hosts nobody has are ignored, a list left empty disappears, st is filled the
 * same way (st may be NULL), and the call waits for the batches in flight.  No list is read back: one
 * pass over the 9 key bytes of every selected posting marks the hits (the host set is searched in LDS
 * up to YRWI_HOST_LDS_MAX hosts, in global memory above), then the lists that lose rows are compacted
 * in chunks of whole lists of at most YRWI_RM_CHUNK rows (environment, read per call; default
 * 67,108,864, at least 256, at most 2^31 - 2; 12 B of scratch per row of the largest chunk), so the
 * call never returns YRWI_E_LIMIT, and st->launches / st->syncs depend on the number of chunks alone.
 * nhosts == 0 or nothing selected: a successful no-op.  YRWI_E_HASH (a host or term hash with a
 * character outside the Base64 alphabet) or YRWI_E_NOMEM: nothing has changed.  A sharded context
 * removes from what it holds; every rank is given the same hosts, and the ranks' `removed` add up. */
#define YRWI_HOST_LDS_MAX 2048
int yrwi_remove_hosts(yrwi_ctx* ctx, const uint8_t* terms12, int32_t nterms, const uint8_t* hosts6,
                      int32_t nhosts, yrwi_update_stats* st);
/* What yrwi_remove_hosts would remove, without changing anything: counts[i] = postings of host i in
 * the selected lists (a host given twice gets its full count twice); *lists_hit = selected lists with at
 * least one such posting (may be NULL).  Errors as yrwi_remove_hosts; a sharded context counts what
 * it holds. */
int yrwi_count_hosts(yrwi_ctx* ctx, const uint8_t* terms12, int32_t nterms, const uint8_t* hosts6,
                     int32_t nhosts, int64_t* counts, int64_t* lists_hit);
/* Census of the hosts: which hosts have postings in the selected lists, and how many each (the front end of
 * yrwi_remove_hosts: the index-wide form of the per-container ConcurrentScoreMap.inc per host hash that
 * ReferenceOrder.doms keeps.  UNVERIFIED against a reference line: the reference has no single method that
 * groups the whole RWI by host).  The selection is yrwi_count_hosts': nterms == 0 every list, otherwise the
 * named lists, duplicates once, unknown terms ignored, an ill-formed term YRWI_E_HASH; the call waits for the
 * batches in flight and changes nothing in the context.  The result is the hosts with at least
 * max(min_postings, 1) postings in the selected lists, in `order`; the first min(hosts_passing, cap) of them
 * are written: hosts6_out + 6 i receives the six characters of the host hash (as yrwi_filter.sitehash),
 * counts_out[i] its postings -- what yrwi_count_hosts returns for that host over the same selection -- and
 * *nout the number written.  cap < hosts_passing is not an error (the top N); cap == 0 with NULL buffers
 * only fills st.  `order` outside the two values, cap < 0, or cap > 0 with a NULL buffer: YRWI_E_ARG; on any
 * error no output buffer is written.  st and nout may be NULL.
 * No list is read back: one streaming pass over the 9 key bytes of every selected posting (k_census, grid and
 * spans as the marking pass of yrwi_remove_hosts) groups them by host, per workgroup in an LDS table of
 * YRWI_CENSUS_LDS_SLOTS slots (environment, read per call, a power of two from 64 to 4096, default 2048) and
 * then in a device table of open addressing (16 B per slot); a posting whose lane finds no place in the LDS
 * table is added to the device table directly (lds_bypass).  The device table starts with the smaller of the
 * next power of two of twice the selected postings and YRWI_CENSUS_SLOTS (environment, read per call, rounded
 * down to a power of two, at least 64, default 4,194,304); a pass that finds no place for a host (within
 * 128 probes) is run again with four times the slots (passes), up to 2^30 slots, beyond which, or when the
 * table cannot be allocated, the call returns YRWI_E_NOMEM.  The hosts that pass are compacted and sorted on
 * the device and only the first min(hosts_passing, cap) cross PCIe.  A sharded context counts what it holds:
 * no collective is involved, every rank is asked the same thing, the ranks' counts of a host add up and the
 * caller merges them.  Per-host distinct url counts are yrwi_host_url_census below; per-host list counts are
 * not part of this. */
#define YRWI_CENSUS_BY_HOST 0   /* ascending host hash (Base64Order of the 6 characters = the 36-bit key order) */
#define YRWI_CENSUS_BY_COUNT 1  /* postings descending; equal counts by ascending host hash */
typedef struct yrwi_census_stats {
  int64_t lists, postings;  /* selected non-empty lists, rows in them: the counts of ALL hosts add up to postings */
  int64_t hosts;            /* distinct hosts in them */
  int64_t hosts_passing;    /* of which with at least min_postings postings: what a cap must hold to get all */
  int64_t table_slots;      /* slots of the device table in the last counting pass */
  int32_t passes;           /* counting passes: 1 + the times the table overflowed and was enlarged */
  int64_t lds_bypass;       /* postings counted straight into the device table (their workgroup's LDS table had no place); last pass */
  int32_t launches, syncs;  /* functions of `passes` (and of `order`: BY_COUNT sorts twice) alone, never of lists, hosts or postings */
  int64_t t_count_ns;       /* device time of the counting passes' k_census launches (HIP events) */
  int64_t t_total_ns;
} yrwi_census_stats;
int yrwi_host_census(yrwi_ctx* ctx, const uint8_t* terms12, int32_t nterms, int32_t order, int64_t min_postings,
                     uint8_t* hosts6_out, int64_t* counts_out, int64_t cap, int64_t* nout, yrwi_census_stats* st);
/* Census of the urls: which documents the selected lists hold, in how many of them each, and how many
 * documents and postings every host has.  UNVERIFIED against a reference line: the reference has no method
 * that groups the whole RWI by url; both calls are defined through calls of this header instead.
 *   Selection: exactly that of yrwi_host_census (nterms == 0 every list, otherwise the named lists, duplicates
 * once, unknown terms ignored).  An ill-formed term or host hash: YRWI_E_HASH with nothing written.  Both calls
 * wait for the batches in flight, bring the url ids up to date as yrwi_build_url_ids does, and otherwise change
 * nothing in the context.
 *   yrwi_url_census: the references of a url are the selected lists that hold a posting of it -- counts[i] of
 * yrwi_url_references over the same selection.  The result is the urls with at least max(min_refs, 1)
 * references and, with nhosts > 0, with url-hash characters 6..11 in the host set (hosts6 + 6 i, as
 * yrwi_remove_hosts takes them: duplicates once, hosts nobody has ignored; the set is sorted and deduplicated
 * on the host, searched in LDS up to YRWI_HOST_LDS_MAX hosts and in global memory above), in `order`.  The
 * first min(urls_passing, cap) are written: urls12_out + 12 i the 12 characters, refs_out[i] the references,
 * *nout the number written.  cap < urls_passing is not an error (the top N); cap == 0 with NULL buffers only
 * fills st.
 *   yrwi_host_url_census: the hosts with at least max(min_urls, 1) distinct urls in the selection, in `order`
 * (YRWI_CENSUS_BY_HOST: ascending host hash; YRWI_CENSUS_BY_COUNT: here distinct urls descending, equal counts
 * by ascending host hash).  hosts6_out + 6 i the host hash, urls_out[i] its distinct urls, postings_out[i]
 * its postings -- what yrwi_host_census reports for that host over the same selection.
 *   `order` outside the two values, cap < 0, or cap > 0 with a NULL buffer: YRWI_E_ARG.  On any error no
 * output buffer and not *nout is written.  st and nout may be NULL.  Nothing selected: a successful empty
 * result that enqueues nothing (st: zeros).  YRWI_E_LIMIT: the limit of the url ids (2^31 postings in the
 * context), or 2^31 - 1 selected postings or dictionary urls or more.
 *   No list is read back and no key is sorted: the group-by runs over the 32-bit url ids of the postings, and
 * ascending id is ascending url hash.  Two ways to count.  YRWI_UCENSUS_HIST: one streaming pass over the
 * 4-byte id of every selected posting (grid and spans of the other maintenance passes) adds 1 to a zeroed
 * 32-bit count per dictionary id; its tail walks the dictionary.  YRWI_UCENSUS_SORT: the selected ids are
 * gathered, radix-sorted over ceil(log2 dict_urls) bits and run-length encoded; its cost follows the selected
 * postings, never the dictionary.  The call takes SORT when postings * UC_SORT_WEIGHT (yrwi_update.hip)
 * <= dict_urls; the environment's YRWI_UCENSUS_PATH = hist | sort, read per call, forces a path; st->path says
 * which ran.  Both paths return the same bytes.  One tail: the urls that pass are flagged, scanned and
 * compacted in id order (YRWI_UCENSUS_BY_URL as it is; BY_REFS: one stable radix sort), the characters of the
 * first min(urls_passing, cap) are written on the device from their dictionary keys, and only those cross
 * PCIe.  The host form sorts the distinct urls by the host of their dictionary key and reduces the runs; the
 * postings are read once.  All scratch is the lane's arena: a steady sequence of calls makes no device-wide
 * allocation after the first.  A sharded context reports what it holds, without a collective: a url lies in
 * one rank's range, so the ranks' urls are disjoint, and a host's url and posting counts add up over the
 * ranks. */
#define YRWI_UCENSUS_BY_URL  0  /* ascending url hash (72-bit key order) */
#define YRWI_UCENSUS_BY_REFS 1  /* references descending; equal references by ascending url hash */
#define YRWI_UCENSUS_HIST 0     /* stats.path: a count per dictionary id */
#define YRWI_UCENSUS_SORT 1     /* stats.path: the selected ids sorted */
typedef struct yrwi_ucensus_stats {
  int64_t lists, postings;  /* selected non-empty lists, rows in them: the references of ALL urls add up to postings */
  int64_t dict_urls;        /* ids of the url dictionary at the call (keys of removed postings stay in it) */
  int64_t urls;             /* distinct urls in the selection, before the host set and the minimum; an id without a selected posting is never counted or returned */
  int64_t urls_hosted;      /* of which with their host in the set; == urls when nhosts == 0 and in the host form */
  int64_t urls_passing;     /* of which with at least min_refs references: what a cap must hold to get all (host form: == urls) */
  int64_t max_refs;         /* the most references of one of the urls_hosted; 0 when there is none */
  int64_t hosts;            /* host form: distinct hosts in the selection */
  int64_t hosts_passing;    /* host form: of which with at least min_urls urls */
  int32_t path;             /* YRWI_UCENSUS_HIST / YRWI_UCENSUS_SORT */
  int32_t launches, syncs;  /* functions of the path, the order and the form alone, never of lists, urls or postings */
  int64_t t_count_ns;       /* device time of the counting kernels (HIP events): k_uc_hist, or gather, sort and run lengths */
  int64_t t_total_ns;
} yrwi_ucensus_stats;
int yrwi_url_census(yrwi_ctx* ctx, const uint8_t* terms12, int32_t nterms, const uint8_t* hosts6, int32_t nhosts,
                    int32_t order, int64_t min_refs, uint8_t* urls12_out, int64_t* refs_out, int64_t cap,
                    int64_t* nout, yrwi_ucensus_stats* st);
int yrwi_host_url_census(yrwi_ctx* ctx, const uint8_t* terms12, int32_t nterms, int32_t order, int64_t min_urls,
                         uint8_t* hosts6_out, int64_t* urls_out, int64_t* postings_out, int64_t cap, int64_t* nout,
                         yrwi_ucensus_stats* st);
/* Retention: keeps the device index inside a budget by two rules on the lastModified day of a posting (the `a`
 * cell: bytes 12-13 of the row, big endian, days; the raw unsigned 16-bit value, not clamped to today -- that
 * clamp belongs to ranking).  UNVERIFIED against a reference line: the reference has no method that drops
 * postings by age or caps a container by age; both rules are defined here.
 *   Selection: that of yrwi_remove_hosts (nterms == 0 every list, otherwise the named lists, duplicates once,
 * unknown terms ignored, an ill-formed term YRWI_E_HASH with nothing changed); both calls wait for the batches
 * in flight.
 *   Age rule: every selected row with a < min_day goes.  min_day is 0 .. 65536: 0 = no age rule, 65536 removes
 * every selected row; outside: YRWI_E_ARG.  A list left empty disappears as after yrwi_put_list(n = 0).
 *   Cap rule: max_refs == 0 = no cap, max_refs < 0: YRWI_E_ARG.  A selected list with s > max_refs survivors of
 * the age rule keeps exactly max_refs of them, those with the largest a: with d* the cut day (the max_refs-th
 * largest a among the survivors), every survivor with a > d* stays, and of the survivors with a == d* the first
 * q = max_refs - |{a > d*}| in url-hash order.  Stated differently: stable-sort the survivors by a descending,
 * keep the first max_refs, restore url-hash order.  The kept rows keep their bytes and their order.
 *   yrwi_retain leaves exactly what yrwi_remove_postings of the removed (term, url) pairs would leave, fills st
 * as that call does (removed == removed_age + removed_cap; st and rst may be NULL) and goes through the same
 * compaction as yrwi_remove_hosts (YRWI_RM_CHUNK).  One pass over the a cells of the selected postings (40 B per
 * posting: the cell sits inside the row) counts the old rows per list; the counts are read back once, and from
 * them the host knows every list's final length.  The cut days and quotas are found and consumed on the device:
 * a two-level radix select (high byte, then low byte, 2 x 256 bins of 4 B per list over the cap) over the
 * flattened postings of the lists over the cap, then, per compaction chunk, the marks a == d* are scanned
 * for a row's rank among its list's rows of the cut day.  launches and syncs depend on the number of
 * compaction chunks and on which rules are given (max_refs > 0: the search and the second scan per chunk are
 * enqueued whether or not a list is over the cap), never on the lists or their lengths; the host waits as
 * often as in yrwi_remove_hosts.  min_day == 0 && max_refs == 0, or nothing selected: a successful no-op that
 * enqueues nothing and reports zeros (day_min = day_max = -1).  YRWI_E_ARG, YRWI_E_HASH, YRWI_E_NOMEM: nothing
 * has changed.
 *   yrwi_retention_count is the dry run: it changes nothing and fills st with the counts yrwi_retain with the
 * same arguments reports (launches, syncs and the times are the dry run's own; t_select_ns is 0: the counts
 * need no cut day).  With day_hist != NULL (65,536 entries) day_hist[d] = selected rows with a == d, counted
 * before any rule (they sum to st->postings), so that a caller can pick the min_day that reaches a target
 * size; with day_hist the pass also runs for min_day == 0 && max_refs == 0.  The histogram is exact: every
 * workgroup counts in an LDS window of 8192 days around the day of its span's first posting, and a posting
 * whose day is outside the window is added to the device table directly (hist_bypass).
 *   A sharded context: the age rule acts on what the rank holds and the ranks' `removed` add up; max_refs > 0
 * returns YRWI_E_UNSUPPORTED with nothing changed (the cap is of the whole container: the ranks would have to
 * exchange their per-list histograms).  Rules on other cells and a persistent per-list day array are not part
 * of this. */
typedef struct yrwi_retention_stats {
  int64_t lists, postings;        /* selected non-empty lists, rows in them */
  int64_t removed_age;            /* rows with a < min_day */
  int64_t removed_cap;            /* rows the cap takes after the age rule */
  int64_t lists_age, lists_cap;   /* lists that lose rows to each rule (a list may be in both) */
  int64_t emptied_terms;          /* lists the age rule empties */
  int32_t day_min, day_max;       /* smallest / largest a over the selected rows, before any rule; -1, -1 when none */
  int32_t launches, syncs;
  int64_t t_mark_ns, t_select_ns; /* HIP events: the streaming pass over the a cells; the per-list cut-day search */
  int64_t t_total_ns;
  int64_t hist_bypass;            /* day_hist only: rows counted straight into the device table (outside the LDS window) */
} yrwi_retention_stats;
int yrwi_retention_count(yrwi_ctx* ctx, const uint8_t* terms12, int32_t nterms, int32_t min_day, int64_t max_refs,
                         int64_t* day_hist, yrwi_retention_stats* st);
int yrwi_retain(yrwi_ctx* ctx, const uint8_t* terms12, int32_t nterms, int32_t min_day, int64_t max_refs,
                yrwi_update_stats* st, yrwi_retention_stats* rst);
/* References of urls: the read-only form of yrwi_remove_postings -- which postings of the selected lists
 * carry one of the nurls url hashes, how many each url has, and the rows themselves with the term of their
 * list (which words index this url; the rows to move, re-host, re-send or re-add).  UNVERIFIED against a
 * reference line: the reference has no such method (Segment.removeAllUrlReferences re-loads and re-parses
 * the document to learn its words); the call is defined through calls of this header instead.
 *   Selection and url set are those of yrwi_remove_postings: nterms == 0 every list, otherwise the named
 * lists; duplicate terms and urls count once, unknown terms and absent urls are ignored.  A reference is a
 * row of a selected list whose url hash is in the set.  The call waits for the batches in flight and
 * changes nothing in the context.
 *   counts[i] (counts may be NULL) = references of urls12 + 12 i; a url given twice gets its full count
 * twice, as in yrwi_count_hosts.  st->refs, st->lists_hit and st->lists_covered are st->removed, st->terms
 * and st->emptied_terms of yrwi_remove_postings with the same arguments.
 *   cap_refs > 0 fetches: reference r in `order` is written, rows40_out + 40 r = the row as stored, all 40
 * bytes (what yrwi_get_list returns for it), terms12_out + 12 r = the term hash of its list.
 * YRWI_REFS_BY_TERM: lists by ascending term hash (the order yrwi_dump_heap writes them in), within a list
 * by ascending url hash; YRWI_REFS_BY_URL: by ascending url hash (72-bit key order), the references of one
 * url by ascending term hash.  cap_refs == 0 only counts (the buffers may be NULL).  st->refs > cap_refs
 * (cap_refs > 0): YRWI_E_ARG with counts and st filled and not a byte of the two buffers written, the rule
 * of yrwi_term_search_batch.  nurls == 0 or nothing selected: a successful empty result.  YRWI_E_HASH (a url
 * or term hash with a character outside the Base64 alphabet): nothing is written.  `order` outside the two
 * values, cap_refs < 0, or cap_refs > 0 with a NULL buffer: YRWI_E_ARG.  YRWI_E_LIMIT: 2^31 urls or more,
 * 2^31 references or more in YRWI_REFS_BY_URL, or YRWI_REFS_PROBE forced over 2^39 (list, url) pairs or more.
 *   Two ways to find the references.  YRWI_REFS_STREAM: one pass over the 9 key bytes of every selected
 * posting (grid and spans of the marking pass of yrwi_remove_hosts; no row is read), each key searched in
 * the sorted url set, which is staged in LDS up to YRWI_REF_LDS_MAX urls (9 B each) and searched in global
 * memory above.  YRWI_REFS_PROBE: one thread per (selected list, url of the set) searches the list for the
 * url -- one document against every list is a search per list, not a pass over the index.  The call takes
 * PROBE when lists * urls * ceil(log2(mean list length + 1)) search steps, each weighed as
 * REF_PROBE_STEP_KEYS streamed keys (yrwi_update.hip, set at the measured crossover), cost no more than the
 * selected postings; the environment's YRWI_REFS_PATH = stream | probe, read per call, forces a path;
 * st->path says which ran.  The results of the two paths are the same bytes.
 *   Delivery: a count pass leaves one hit count per tile of the path's domain (1024 postings, 256 pairs),
 * one workgroup scans them with a 64-bit carry, and the pack pass finds its hits again in the tiles that
 * have any and writes each at its tile's start plus its rank in the tile; it reads the total from device
 * memory and stores nothing when it exceeds cap_refs, so the host does not wait in between.
 * YRWI_REFS_BY_URL sorts the references alone (never the postings) stably by their slot in the url set
 * on the device.  rows40_out from yrwi_host_alloc and 8-byte aligned is written by the kernel itself
 * (st->direct = 1); any other buffer receives the rows from device scratch through the lane's pinned
 * landing buffer.  Scratch grows with the tiles and with min(cap_refs, lists * urls, postings), never with
 * the postings alone.  st->launches / st->syncs depend on the order, on count-only against fetch and on
 * direct alone: 4 / 2 counting; fetching 8 / 3 by term and 10 / 3 by url, one launch fewer when direct.
 * A steady sequence of calls makes no device-wide allocation after the first.  A sharded context reports
 * what it holds: every rank gets the same call, no collective runs, a url lies in one rank's range, so the
 * ranks' references are disjoint and their counts add up.  st may be NULL. */
#define YRWI_REFS_BY_TERM 0   /* term ascending (the order yrwi_dump_heap writes lists in), then url hash ascending */
#define YRWI_REFS_BY_URL  1   /* url hash ascending (72-bit key order), then term ascending */
#define YRWI_REFS_STREAM  0   /* stats.path: one pass over the selected postings' keys */
#define YRWI_REFS_PROBE   1   /* stats.path: one search per (selected list, url) */
#define YRWI_REF_LDS_MAX 2048
typedef struct yrwi_ref_stats {
  int64_t lists, postings;    /* selected non-empty lists, rows in them */
  int64_t urls, urls_found;   /* distinct urls given; of which with at least one reference */
  int64_t refs;               /* references found == st->removed of yrwi_remove_postings with the same arguments */
  int64_t lists_hit;          /* == st->terms of that call */
  int64_t lists_covered;      /* lists all of whose rows are references == st->emptied_terms of that call */
  int32_t path, direct;       /* path taken; 1: the kernel wrote the rows into the caller's buffer */
  int32_t launches, syncs;
  int64_t bytes_h2d, bytes_d2h;
  int64_t t_find_ns, t_total_ns;
} yrwi_ref_stats;
int yrwi_url_references(yrwi_ctx* ctx, const uint8_t* terms12, int32_t nterms, const uint8_t* urls12, int64_t nurls,
                        int32_t order, int64_t* counts, uint8_t* terms12_out, uint8_t* rows40_out, int64_t cap_refs,
                        yrwi_ref_stats* st);
/* Brings the url dictionary (url hash -> order-preserving 32-bit url id, the
 * join key in HBM) up to date now instead of at the next query.  The first
 * build sorts every key; later put_list / removal / load_heaps changes are
 * merged in incrementally (IndexCell.add, IndexCell.java:289): only the changed
 * lists' keys are sorted, keys new to the dictionary shift the ids after them
 * (the other lists' ids are remapped in one pass, not re-sorted), and keys of
 * removed postings stay until a full rebuild (when the changed lists hold over
 * a quarter of the postings, or removed ones over half; YRWI_DICT_FULL=1
 * forces it). */
int yrwi_build_url_ids(yrwi_ctx* ctx);
/* Diagnostic: brings the ids up to date, then *bad = postings whose id does not
 * name their url hash or does not ascend within its list, plus dictionary
 * entries out of order (0 when consistent); *nurls = dictionary size (may be NULL). */
int yrwi_check_url_ids(yrwi_ctx* ctx, int64_t* bad, int64_t* nurls);
int yrwi_index_stats(yrwi_ctx* ctx, int64_t* nterms, int64_t* npostings, int64_t* device_bytes);
/* Index maintenance counters (diagnostics and tests). */
typedef struct yrwi_index_info {
  int64_t full_rebuilds;        /* url dictionary built from every key */
  int64_t incremental_updates;  /* changed lists merged into an existing dictionary */
  int64_t repacks;              /* index memory compactions (dead bytes of replaced lists reclaimed) */
  int64_t index_bytes;          /* device bytes of the index arena (rows, keys, records, incremental ids) */
  int64_t index_bytes_used;     /* of which allocated so far (live + not yet reclaimed) */
  int64_t bitmap_lists;         /* lists with a url-id bitmap */
} yrwi_index_info;
int yrwi_index_info_get(yrwi_ctx* ctx, yrwi_index_info* info);
/* The pair cache: the joined containers of two-term queries (two distinct include
 * terms, no exclude term, no filter, no url selection, max_distance
 * YRWI_MAX_DISTANCE_ANY, no authority profile; yrwi_query / yrwi_query_batch and
 * their rows and submit forms on an unsharded context) are kept in device memory
 * across calls, keyed by the two terms and the day now_ms falls on.  A later query
 * of the pair skips its join and is normalised, scored and cut from the kept
 * container: results do not change.  Every index change drops all entries.
 * Environment, read per call: YRWI_PAIR_CACHE=0 turns it off; YRWI_PAIR_CACHE_MB
 * (default 2048) is the byte budget -- the device block itself is reserved when the
 * url ids are next built (after an index change; a context whose ids were built
 * with the cache off, or with a smaller value, has no or a smaller block until
 * then), later calls may only lower the budget within it;
 * YRWI_PAIR_CACHE_MIN_ROWS (default 16384) is the joined size from which a
 * container is kept.  The counters run from yrwi_open. */
typedef struct yrwi_pair_cache_info {
  int64_t enabled;         /* 1: query batches use it (0: switched off, a sharded context, or no block reserved yet) */
  int64_t capacity_bytes;  /* the device block */
  int64_t budget_bytes;    /* of which entries may take now */
  int64_t min_rows;        /* admission minimum now */
  int64_t entries;         /* containers a query can find */
  int64_t pieces;          /* their normalisation pieces (one per tile of the join that wrote them), summed */
  int64_t bytes;           /* of the block in use */
  int64_t hits;            /* queries served from an entry */
  int64_t misses;          /* queries the cache serves that found none (lists shorter than min_rows are not looked up) */
  int64_t fills;           /* entries written */
  int64_t dropped;         /* fills given up: another lane had filled the key meanwhile */
  int64_t evictions;       /* entries displaced by a fill, least recently used first */
  int64_t invalidations;   /* times an index change dropped every entry (a change that finds none is not counted) */
  int64_t rows_served;     /* joined rows of all hits */
} yrwi_pair_cache_info;
int yrwi_pair_cache_info_get(yrwi_ctx* ctx, yrwi_pair_cache_info* info);
/* Device-wide allocation events of the process so far (scratch arena growth,
 * pinned staging growth: each one stalls every lane of the device while it
 * runs).  A caller counts them around a timed region without per-batch
 * statistics; steady-state batches make none. */
int64_t yrwi_realloc_events(void);
/* Sizes every lane's scratch arena and pinned staging to the largest any lane has
 * needed so far (one allocation each): call after a few representative batches,
 * and later batches of that workload make no device-wide allocation on any lane
 * (a lane otherwise grows on its own first large batch). */
int yrwi_settle_scratch(yrwi_ctx* ctx);
/* Diagnostic of the node's shared-memory size exchange (no GPU needed): rank
 * `rank` of `world` processes / threads sharing group id `id` runs `nparts`
 * batch parts of `ncalls` exchanges each, vectors of n values (rank + part +
 * call + i), and checks every sum.  0 when all sums are right; YRWI_E_RCCL on a
 * wrong sum or a peer that never arrives; 1 when the mailbox is unavailable.
 * n < 0 (vectors of -n values): the last rank's first part fails and aborts the
 * mailbox, as a failing batch part does; the others return YRWI_E_RCCL at once. */
int yrwi_hostx_selftest(const uint8_t id[128], int world, int rank, int64_t nparts, int32_t ncalls, int64_t n);

/* ---- YaCy on-disk index ---- */
/* Loads BLOB heap files of the RWI (records [int32 reclen][12-byte term hash]
 * [exported RowSet], HeapWriter.java:114-124, RowCollection.java:209-224) into
 * device memory.  Files are folded oldest first with RowSet.mergeEnum (the older
 * file's row wins on equal url hashes; ReferenceContainerArray.get :305-322);
 * lists already in the context act as the RAM cache and are merged below the
 * files (IndexCell.get :353-386).  A sharded context keeps only its url-hash
 * range.  With YRWI_LOAD_ORDER_BY_NAME the files are ordered by the
 * <prefix>.<yyyyMMddHHmmssSSS>.blob stamp and others are ignored
 * (ArrayStack.java:182-229); otherwise `paths` is taken as oldest first.
 * Malformed records are skipped as HeapReader does; a term whose RowSet export
 * is inconsistent (importRowSet's SpaceExceededException) keeps only its RAM
 * list, as does a term with malformed rows (a url hash outside the alphabet, an
 * empty language cell, or rows that claim to be sorted, orderbound >= size, and do
 * not ascend strictly; rows past orderbound are sorted, the first of equal url
 * hashes stays, and every one of them is checked); both are counted in
 * dropped_terms. */
#define YRWI_LOAD_ORDER_BY_NAME 1
typedef struct yrwi_load_stats {
  int64_t files, records, free_records, bad_keys;
  int64_t terms;          /* lists stored (replaced or new) */
  int64_t postings;       /* rows in those lists */
  int64_t dropped_terms;
} yrwi_load_stats;
int yrwi_load_heaps(yrwi_ctx* ctx, const char* const* paths, int32_t npaths, int32_t flags,
                    yrwi_load_stats* st);

/* Two cells of the 14-byte export header that yrwi_dump_heap writes are UNVERIFIED against the
 * reference source (written from memory; no reader here or, per SURVEY.md §8f.1, in the reference
 * depends on either):
 *   - orderkey: the two bytes "Be", Base64Order.enhancedCoder.signature();
 *   - lastread / lastwrote: whole days from 2000-01-01T00:00:00Z to the call's time. */
#define YRWI_DUMP_ORDERKEY0 'B'
#define YRWI_DUMP_ORDERKEY1 'e'
#define YRWI_DUMP_EPOCH_MS 946684800000LL /* 2000-01-01T00:00:00Z in ms since 1970 */
typedef struct yrwi_dump_stats {
  int64_t terms, postings;  /* records written, rows in them */
  int64_t bytes;            /* file size */
  int64_t windows;          /* windows of the file image packed on the device */
  int32_t launches;         /* kernel launches, copies and memsets enqueued: a function of bytes and the
                               window size, never of the number of terms */
  int32_t syncs;            /* host waits on the device: a function of the number of windows only */
  int64_t t_pack_ns;        /* device time of the pack kernels (HIP events) */
  int64_t t_total_ns;
} yrwi_dump_stats;
/* ReferenceContainerCache.dump / the FlushThread dump of IndexCell (IndexCell.java:131-166) through
 * HeapWriter.add (HeapWriter.java:114-124) and RowCollection.exportCollection (:209-224): writes the
 * context's lists to one BLOB heap file that yrwi_load_heaps (and a stock HeapReader) reads back.
 * nterms == 0: every list; otherwise the named lists (duplicates count once, unknown terms are
 * ignored; an ill-formed term: YRWI_E_HASH, nothing written).  The file is the concatenation, in
 * Base64Order of the term hashes, of one record per non-empty list:
 *   [int32 BE reclen = 12 + 14 + 40 n][12-B term hash][export header][n rows of 40 B as stored],
 * export header = size n (int32 BE), lastread and lastwrote (int16 BE: days from 2000-01-01 to
 * now_ms; now_ms == 0: now), orderkey "Be", orderbound n (int32 BE).  No lists or an empty
 * selection: a 0-byte file.  The .idx / .gap companions are not written (HeapReader rebuilds its
 * index by scanning the file).  The bytes go to <path>.prt, renamed onto `path` after the last
 * byte is written and flushed; on any failure the temporary file is removed and an existing
 * `path` is untouched (file errors: YRWI_E_IO, strerror text in yrwi_last_error).
 * The file image is packed on the device in windows of YRWI_DUMP_WINDOW bytes (environment, read
 * per call, rounded down to a multiple of 256, at least 256, at most 1 GiB; default 32 MiB); extra
 * device memory is two windows and the job table, whatever the index size.  The call waits for the
 * batches in flight, as yrwi_get_list does, and changes nothing in the context.  A sharded context
 * writes the lists it holds, i.e. its url-hash range of every term: no collective is involved,
 * the shards' files cover disjoint url ranges and loaded together give the whole index.
 * st may be NULL. */
int yrwi_dump_heap(yrwi_ctx* ctx, const char* path, const uint8_t* terms12, int32_t nterms,
                   int64_t now_ms, yrwi_dump_stats* st);

/* ---- DHT send path (yrwi_dht.hip): select, split and remove containers on the device ----
 * Dispatcher.selectContainersEnqueueToBuffer: selectContainers walks the term order from a start
 * hash and takes whole containers up to a container and a reference count, IndexCell.remove(termHash)
 * takes them out of the index, and splitContainers / splitContainer divide each one by
 * Distribution.verticalDHTPosition(urlhash) into 2^e partitions, which Transmission sends to the
 * partitions' target peers.
 * Three things here are UNVERIFIED against the reference source (written from memory):
 *   - Word.isPrivate(termHash): the hash starts with the two bytes YRWI_DHT_PRIVATE0/1 ("_C");
 *   - the first container is taken even when its term is >= limit;
 *   - after a wrap the term is still compared with a plain `< limit`. */
#define YRWI_DHT_ROT 1           /* referenceContainerIterator(hash, rot = true): wrap to the smallest term */
#define YRWI_DHT_REMOVE 2        /* remove the selected lists from the index once their rows have landed */
#define YRWI_DHT_SKIP_PRIVATE 4  /* Word.isPrivate(termHash) containers are passed over, uncounted */
#define YRWI_DHT_COUNT_ONLY 8    /* dry run: fill st only, change nothing */
#define YRWI_DHT_MAX_EXPONENT 8
#define YRWI_DHT_PRIVATE0 '_'    /* UNVERIFIED, see above */
#define YRWI_DHT_PRIVATE1 'C'
typedef struct yrwi_dht_stats {
  int64_t terms, postings;      /* containers selected, rows in them (also the capacities a retry needs) */
  int64_t skipped_private;
  int64_t removed;              /* postings removed from the index */
  int32_t wrapped;              /* the walk passed the end of the term order and went on at the smallest term */
  int64_t windows;
  int32_t launches, syncs;      /* functions of postings / window size and 2^e, never of the number of terms */
  int64_t t_pack_ns, t_total_ns;
} yrwi_dht_stats;
/* Selection: the context's non-empty lists in Base64Order of their term hashes, from the first term
 * >= start; with YRWI_DHT_ROT the walk goes on at the smallest term after the largest and stops after
 * one full cycle (no term twice), without it at the end.  The next list is taken while
 * selected < max_containers, refs < max_refs, and nothing is selected yet or its term is < limit
 * (a plain key comparison, also after a wrap): so the first container is taken whatever `limit` is,
 * the last one may push refs past max_refs, and max_containers <= 0 or max_refs <= 0 select nothing
 * (rc 0).  With YRWI_DHT_SKIP_PRIVATE a private term is passed over: it does not count and does not
 * end the walk.  There is no time limit.
 * Split: P = 2^partition_exponent (0 .. YRWI_DHT_MAX_EXPONENT); a posting's partition is the top e
 * bits of its 72-bit url key -- for e <= 6 the shard rule of yrwi_open_shard.
 * Output, T the number of selected terms: terms12_out receives the T term hashes in selection order;
 * part_off (room for P * cap_terms + 1 entries) receives P * T + 1 non-decreasing row offsets in
 * partition-major order: the rows of term j in partition p are rows40_out + 40 * part_off[p * T + j]
 * up to part_off[p * T + j + 1], in url-hash order and byte-identical to what yrwi_get_list returns;
 * part_off[P * T] == st->postings.  rows40_out may be yrwi_host_alloc memory: when it is and is
 * 8-byte aligned the rows land in it directly, else through a pinned window.
 * The boundaries of every (list, partition) are searched in one launch and summed in one device
 * scan; the rows are packed in windows of YRWI_DHT_WINDOW_ROWS rows (environment, read per call;
 * default 1,048,576, at least 16, at most 2^24), two device and two pinned windows shared with
 * yrwi_dump_heap.  Extra device memory is the windows, the job table and the P * T cells.
 * Every failure leaves the index unchanged and writes no output buffer, st excepted where said:
 * cap_terms < T or cap_rows < postings: YRWI_E_ARG, st->terms and st->postings filled for a retry;
 * an ill-formed start or limit: YRWI_E_HASH; e out of range or unknown flag bits: YRWI_E_ARG;
 * YRWI_E_NOMEM, YRWI_E_HIP (rows of windows already landed may have been written).
 * With YRWI_DHT_REMOVE the lists are erased only after the last row has landed, as
 * yrwi_remove_hosts erases a list it empties; their memory is reclaimed by the next repack.  The
 * caller puts back what it could not send with yrwi_add_postings(YRWI_ADD_KEEP).
 * YRWI_DHT_COUNT_ONLY fills st with what the same call would select and touches neither the buffers
 * (which may be NULL) nor the index.  The call waits for the batches in flight, as yrwi_put_list
 * does.  A sharded context selects from the lists it holds, its url range of each term: no
 * collective is involved, and the cells of partitions outside its range come out empty.
 * st may be NULL. */
int yrwi_dht_select(yrwi_ctx* ctx, const uint8_t start[12], const uint8_t limit[12],
                    int32_t max_containers, int64_t max_refs, int32_t partition_exponent, int32_t flags,
                    uint8_t* terms12_out, int32_t cap_terms, int64_t* part_off,
                    uint8_t* rows40_out, int64_t cap_rows, yrwi_dht_stats* st);

/* ---- query hot path ---- */
/* TermSearch + joinExcludeContainers + normalizeWith + cardinal + rwiStack top-k
 * (SearchEvent.RWIProcess.run :612-631 -> addRWIs :673-836), canonical
 * deterministic semantics.  out: k hits, best first. */
int yrwi_query(yrwi_ctx* ctx, const yrwi_query_desc* q, yrwi_hit* out, int32_t* nout, yrwi_stats* st);
/* nq independent queries in one device pass (throughput mode).
 * out: nq * kmax hits (row q at out + q*kmax), nout[q] = hits of query q. */
int yrwi_query_batch(yrwi_ctx* ctx, const yrwi_query_desc* q, int32_t nq, int32_t kmax,
                     yrwi_hit* out, int32_t* nout, yrwi_stats* st);

/* Asynchronous batches (throughput mode: SearchEvent runs many RWIProcess
 * feeders concurrently, SearchEvent.java:612-631).  submit returns at once with
 * a ticket; the batch runs on one of the context's lanes (own HIP stream and
 * host thread) while the caller prepares the next one.  q, the profiles it
 * points to, out, nout and st must stay valid until yrwi_query_batch_wait(ticket)
 * returns; every ticket must be waited for exactly once.  Lists must not be
 * changed while batches are in flight (put_list waits for them).  Sharded
 * contexts: every rank submits the same batches in the same order (the batches'
 * device collectives are enqueued in submission order). */
int yrwi_query_batch_submit(yrwi_ctx* ctx, const yrwi_query_desc* q, int32_t nq, int32_t kmax,
                            yrwi_hit* out, int32_t* nout, yrwi_stats* st, int64_t* ticket);
int yrwi_query_batch_wait(yrwi_ctx* ctx, int64_t ticket);

/* The query path with the joined posting of every hit (SearchEvent.rwiStack holds the
 * WordReferenceVars of the joined posting, which pullOneRWI hands to Fulltext.getMetadata,
 * SearchEvent.java:1297-1394): out and nout are exactly what yrwi_query / yrwi_query_batch /
 * yrwi_query_batch_submit return for the same batch, and rows40_out (nq * kmax * 40 bytes; one
 * query: k rows) receives the 40-byte row of hit i of query q at rows40_out + (q * kmax + i) * 40,
 * i < nout[q]; the bytes past a query's nout[q] rows are unspecified.  The row is the one
 * yrwi_term_search writes for the hit's url under the same descriptor: one include term, the
 * list's row as stored (typeofword, reserve and freshUntil included); two or more, the joined
 * record as toRowEntry re-encodes it (typeofword and reserve 0, freshUntil from the query's
 * now_ms).  Filters, the doubledom pull order, urlselection, max_distance and exclusions decide
 * which hits there are and their order, never a row's bytes.  rows40_out == NULL: the call is
 * its counterpart without rows.  The rows go where the hits go: straight into rows40_out when it
 * came from yrwi_host_alloc and is 8-byte aligned, else through the lane's landing buffer; like
 * out it must stay valid until yrwi_query_batch_wait returns (submit).
 * Sharded contexts (yrwi_open_shard): every rank ends with the same hits; a rank writes the rows
 * of the hits whose url hash lies in its own range -- the first character's index c with
 * c >> (6 - log2(world)) == rank (Distribution.java:153-158) -- and 40 zero bytes for the hits
 * another rank owns.  No collective is added: the ranks' rows are disjoint and together give the
 * row of every hit. */
int yrwi_query_rows(yrwi_ctx* ctx, const yrwi_query_desc* q, yrwi_hit* out, uint8_t* rows40_out, int32_t* nout,
                    yrwi_stats* st);
int yrwi_query_batch_rows(yrwi_ctx* ctx, const yrwi_query_desc* q, int32_t nq, int32_t kmax, yrwi_hit* out,
                          uint8_t* rows40_out, int32_t* nout, yrwi_stats* st);
/* collected with yrwi_query_batch_wait */
int yrwi_query_batch_rows_submit(yrwi_ctx* ctx, const yrwi_query_desc* q, int32_t nq, int32_t kmax, yrwi_hit* out,
                                 uint8_t* rows40_out, int32_t* nout, yrwi_stats* st, int64_t* ticket);

/* Pinned host memory for result buffers: hits written into such a buffer come
 * straight from the GPU (no staging copy).  Free with yrwi_host_free. */
int yrwi_host_alloc(yrwi_ctx* ctx, size_t bytes, void** p);
int yrwi_host_free(yrwi_ctx* ctx, void* p);

/* ---- Solr node stack ---- */
/* The fields of a URIMetadataNode that ReferenceOrder.cardinal(URIMetadataNode)
 * reads (ReferenceOrder.java:267-296); the caller extracts them from the Solr
 * document (URIMetadataNode.java:238-504). */
typedef struct yrwi_node {
  uint8_t urlhash[12];    /* t.hash() */
  int32_t virtual_age;    /* t.virtualAge() = MicroDate.microDateDays(moddate) */
  int32_t wordsintitle;   /* t.wordsintitle() */
  int32_t wordcount;      /* t.wordCount() */
  int32_t llocal, lother; /* t.llocal(), t.lother() */
  uint8_t flags[4];       /* t.flags() Bitfield bytes */
  int32_t host_count;     /* ReferenceOrder.doms.get(t.hosthash()) (authority) */
  char language[8];       /* t.language(), NUL terminated; "" = null */
} yrwi_node;
/* scores[i] = cardinal(nodes[i]) under `prof` and the ReferenceOrder language;
 * maxdomcount is ReferenceOrder.maxdomcount (authority divisor 1 + maxdomcount). */
int yrwi_score_nodes(yrwi_ctx* ctx, const yrwi_node* nodes, int64_t n, const yrwi_profile* prof,
                     const char* language, int32_t maxdomcount, int64_t* scores);

/* ---- search events: local + remote containers merged per arrival ---- */
/* A SearchEvent's RWI side (SearchEvent.java:673-836): containers arrive one
 * after another -- the local joined container from RWIProcess.run (:612-631) and
 * each remote peer's result container from Protocol.remoteSearchProcess
 * (Protocol.java:670-830, addRWIs(container, false, ...) at :802).  Every
 * arrival continues the event's ReferenceOrder (min/max, max-distance fold,
 * host counts), is settled over itself and then scored; entries already on the
 * stack keep their arrival-time scores.  The doublecheck set (SearchEvent.
 * urlhashes), the flag counts and the rwiStack (bound k) persist in device
 * memory.  Rows are WordReferenceRow bytes in the container's order (a remote
 * container is in the order the peer's results arrived). */
typedef struct yrwi_event yrwi_event;
/* k: stack bound (<= YRWI_MAX_K; the results kept); filter: constraints, its
 * urlhashes seed the doublecheck set (NULL: unconstrained; its flagcount and
 * skip_double_dom are not used -- see yrwi_event_result, yrwi_event_pull); max_postings: the
 * most postings the event will receive (sizes the url and host tables). */
int yrwi_event_open(yrwi_ctx* ctx, const yrwi_profile* prof, const char* language, int64_t now_ms, int32_t k,
                    const yrwi_filter* filter, int64_t max_postings, yrwi_event** out);
/* An event for yrwi_event_order / yrwi_event_authority only (GpuReferenceOrder: the
 * ReferenceOrder of a SearchEvent whose addRWIs stays in Java): no url set and no
 * stack, the host table first sized for max_hosts distinct hosts (authority
 * profiles) and grown by yrwi_event_order before a container could fill it
 * (ReferenceOrder.doms is unbounded, ReferenceOrder.java:176-198), device memory
 * reused from closed order-only events.
 * The event entry points serialise on the context (callers on several threads). */
int yrwi_event_open_order(yrwi_ctx* ctx, const yrwi_profile* prof, const char* language, int64_t now_ms,
                          int64_t max_hosts, yrwi_event** out);
typedef struct yrwi_arrival {
  yrwi_event* ev;
  const uint8_t* rows40;  /* n rows of 40 bytes */
  int64_t n;
  int32_t local;          /* addRWIs(local): statistics only */
  int32_t rc;             /* out: 0 or YRWI_E_* (HASH, NULL_LANGUAGE, CAPACITY) for this arrival */
} yrwi_arrival;
/* Applies arrivals in array order (per event); arrivals of different events run
 * in parallel, one workgroup per event.  Returns the first nonzero rc. */
int yrwi_event_add(yrwi_ctx* ctx, yrwi_arrival* arr, int32_t narr);
/* ReferenceOrder.normalizeWith(container, local) + cardinal of each of its rows
 * for a drop-in ReferenceOrder whose SearchEvent.addRWIs stays in Java
 * (ReferenceOrder.java:70-79,163-265; GpuReferenceOrder): the container continues
 * the event's ReferenceOrder exactly as an arrival does -- min/max and the
 * max-distance fold accumulate over every container given so far, the host counts
 * (doms, maxdomcount) too -- and scores[i] = cardinal(row i) under the state after
 * this container (settled over it).  The event's doublecheck set,
 * flag counts and stack are not touched (addRWIs keeps its own).  Do not mix
 * with yrwi_event_add on one event. */
int yrwi_event_order(yrwi_ctx* ctx, yrwi_event* ev, const uint8_t* rows40, int64_t n, int32_t local,
                     int64_t* scores);
/* ReferenceOrder.authority(hostHash) (ReferenceOrder.java:213-216) against the
 * event's accumulated host counts: out[i] = (doms(h_i) << 8) / (1 + maxdomcount),
 * h_i the 6-character host hash at hosts6 + 6 i (url-hash chars 6..11).  The
 * counts exist when the event's profile has coeff_authority > 12 (else 0). */
int yrwi_event_authority(yrwi_ctx* ctx, yrwi_event* ev, const uint8_t* hosts6, int32_t n, int32_t* out);
typedef struct yrwi_event_info {
  int32_t flagcount[32];        /* SearchEvent.flagcount */
  int64_t postings_in;          /* rows received */
  int64_t admitted_local;       /* local_rwi_available */
  int64_t admitted_remote;      /* remote_rwi_available */
  int64_t remote_arrivals;      /* remote_rwi_peerCount */
  int32_t maxdomcount;          /* ReferenceOrder.maxdomcount (authority profiles only) */
  int32_t max_distance;         /* max.distance() of the fold (min.distance() is 0) */
  int32_t err;                  /* YRWI_E_CAPACITY once the event's tables overflowed */
  int32_t stack_size;
} yrwi_event_info;
/* Where each url entered the event's doublecheck set (SearchEvent.urlhashes,
 * :736-805: the first posting of the url that passed the constraints):
 * arrival[i] = its yrwi_event_add arrival (1 = the event's first), row[i] = its row
 * in that arrival's rows; arrival 0 (row 0) = seeded by the filter's urlhashes; -1
 * (row -1) = not in the set.  The numbers count the arrivals that were applied: an
 * empty arrival (n = 0) and a rejected one (rc != 0) use none up, as an empty
 * yrwi_event_add_local join.  A caller that keeps the rows of the arrivals it got
 * applied (GpuRWIStack) turns a pulled hit back into its posting. */
int yrwi_event_source(yrwi_ctx* ctx, yrwi_event* ev, const uint8_t* urls12, int32_t n, int32_t* arrival,
                      int32_t* row);
/* The stack in rwiStack order (best first), up to maxn entries. */
int yrwi_event_result(yrwi_ctx* ctx, yrwi_event* ev, yrwi_hit* out, int32_t maxn, int32_t* nout,
                      yrwi_event_info* info);
/* SearchEvent.pullOneRWI(skip_double_dom) (SearchEvent.java:1297-1394) repeated
 * up to maxn times, stopping where it returns null: each pull polls the event's
 * rwiStack (the entry leaves it, so later arrivals fill the bound again); with
 * skip_double_dom, an entry whose host was already returned goes to that host's
 * doubleDomCache queue, and after 10 such polls (or an empty stack) the best head
 * of those queues is returned (a host whose queue empties leaves the cache).  The
 * cache persists across calls and arrivals.  Equal heads of different hosts go
 * by ReverseElement order, then the earliest queued (the reference walks a
 * ConcurrentHashMap).  Every url is taken to have metadata (the fulltext lookup
 * at :1309,1327,1392 is not on the RWI path). */
int yrwi_event_pull(yrwi_ctx* ctx, yrwi_event* ev, int32_t skip_double_dom, yrwi_hit* out, int32_t maxn,
                    int32_t* nout);
/* ---- the local container of a search event, straight from the device index ----
 * RWIProcess.run hands TermSearch's joined container to addRWIs(container, local = true)
 * (SearchEvent.java:612-631; the sitehost retry at :651 a second time).  A device-local
 * arrival is that pair of steps without the rows leaving the device: the event ends in
 * exactly the state that yrwi_term_search(ctx, q, rows, cap, &m) followed by yrwi_event_add
 * of {ev, rows, m, local = 1} leaves -- stack, doublecheck set, flag counts, ReferenceOrder,
 * host counts, yrwi_event_info and yrwi_event_source answers -- and later yrwi_event_add
 * arrivals continue from it. */
typedef struct yrwi_local_arrival {
  yrwi_event* ev;
  const yrwi_query_desc* q; /* incl, excl, max_distance, now_ms, urlselection: as yrwi_term_search reads them;
                               k, profile, language, filter unused (the event has its own) */
  int64_t m;                /* out: rows of the joined and excluded container that arrived */
  int32_t rc;               /* out: 0 or YRWI_E_* for this arrival (CAPACITY) */
} yrwi_local_arrival;
typedef struct yrwi_local_stats {
  int64_t rows_joined, rows_arrived; /* before / after exclusion, summed over the call */
  int64_t bytes_h2d, bytes_d2h;      /* bytes the call moved over PCIe: descriptors, tables, statuses -- never rows */
  int32_t launches_tail;             /* launches, copies and memsets enqueued after the join phase */
  int32_t syncs;                     /* host waits on the device in the whole call */
  int64_t t_total_ns;
  int64_t device_allocs;             /* device-wide allocation events of the call (yrwi_realloc_events): the one
                                        block of retained rows, none for a call whose containers are all empty */
} yrwi_local_stats;
/* Applies the arrivals in array order within an event; arrivals of different events run in
 * parallel, one workgroup per event, as yrwi_event_add does.  The containers of all arrivals
 * are joined in one pass, turned into rows on the device (k_local_rows) and read by
 * k_event_add where they lie: no row crosses PCIe, and launches_tail and syncs do not depend
 * on narr.  An absent include term or an empty join gives m = 0, rc = 0 and leaves the event
 * as it is (no arrival number is used up).  Planning errors (YRWI_E_HASH, YRWI_E_UNSUPPORTED
 * urlselection cases, YRWI_E_ARG -- an event from yrwi_event_open_order included --,
 * YRWI_E_NOMEM) return before anything is applied to any event; YRWI_E_CAPACITY is reported
 * per arrival in rc and the first nonzero rc is returned.  A context of a shard group
 * (yrwi_open_shard with world > 1) returns YRWI_E_UNSUPPORTED: a shard holds only its url
 * range of the container, and events are not combined across ranks.  Waits for batches in
 * flight and serialises with the other event entry points.  st may be NULL.
 * The arrivals' rows stay in device memory (one allocation per call, 40 bytes per joined
 * row, shared by the events of the call) until the last of those events closes or the
 * context does: yrwi_event_rows reads them. */
int yrwi_event_add_local(yrwi_ctx* ctx, yrwi_local_arrival* arr, int32_t narr, yrwi_local_stats* st);
/* The posting of each url at urls12 + 12 i as the event admitted it (its doublecheck set,
 * as yrwi_event_source): found[i] = 1 and the row at rows40_out + 40 i when that posting
 * arrived through yrwi_event_add_local; found[i] = 0 and 40 zero bytes for a url that is not
 * in the set, was seeded by the filter, or was admitted from a yrwi_event_add arrival (whose
 * rows the caller holds).  A hit taken by yrwi_event_pull stays in the set, so its row is
 * still found.  rows40_out may be yrwi_host_alloc memory (written directly when 8-byte
 * aligned). */
int yrwi_event_rows(yrwi_ctx* ctx, yrwi_event* ev, const uint8_t* urls12, int32_t n, uint8_t* rows40_out,
                    uint8_t* found /* n bytes */);
void yrwi_event_close(yrwi_ctx* ctx, yrwi_event* ev);

/* ---- index abstracts and the secondary search ---- */
/* AbstractIndex.searchConjunction + WordReferenceFactory.compressIndex for each
 * term (htroot/yacy/search.java:264-281, SearchEvent.java:505-531;
 * WordReferenceFactory.java:75-117 without its time limit): "{host:u6u6...,host:...}"
 * with hosts in String order and url prefixes in container order, minus the urls
 * of exclude_term's list (NULL: none).  Abstract i is out[offsets[i],
 * offsets[i+1]); *nout = nterms, or 0 when a term has no list (searchConjunction
 * returns no containers then). */
int yrwi_index_abstracts(yrwi_ctx* ctx, const uint8_t* terms, int32_t nterms, const uint8_t* exclude_term,
                         char* out, int64_t cap, int64_t* offsets, int32_t* nout);
/* One index abstract received from a peer (Protocol.java:576-596). */
typedef struct yrwi_abstract {
  uint8_t word[12];
  uint8_t peer[12];
  const char* text;
  int64_t len;
} yrwi_abstract;
/* A secondary search request (SecondarySearchSuperviser.prepareSecondarySearch
 * :117-196): the peer, the words to ask it for (bit i = words_out[i]) and its urls
 * (plan_urls[url_off .. url_off + url_n), 12 bytes each, String order). */
typedef struct yrwi_peer_request {
  uint8_t peer[12];
  uint32_t words;
  int64_t url_off, url_n;
} yrwi_peer_request;
/* decompressIndex of every abstract (in arrival order), addAbstract, the
 * joinConstructive of the words and the requests for the peers other than
 * mypeer and `checked` (SecondarySearchSuperviser.java:43-196, WordReferenceFactory.
 * java:125-155, SetTools.java:76-116).  Nothing is planned unless the abstracts
 * cover exactly nwords_query words.  Outputs: the join (njoin urls in String
 * order with their peer), words_out (the words in String order, <= 32), the
 * requests in peer order.  A text that is not a compressIndex abstract fails with
 * YRWI_E_ARG (the reference would read past its buffer); one without braces is
 * an empty abstract. */
int yrwi_secondary_search(yrwi_ctx* ctx, const yrwi_abstract* abs, int32_t nabs, int32_t nwords_query,
                          const uint8_t mypeer[12], const uint8_t* checked, int32_t nchecked,
                          uint8_t* join_urls, uint8_t* join_peers, int64_t cap, int64_t* njoin,
                          yrwi_peer_request* plan, int32_t plan_cap, int32_t* nplan, uint8_t* plan_urls,
                          uint8_t* words_out, int32_t* nwords);

/* ---- finer-grained drop-ins mirroring the Java split ---- */
/* == ReferenceContainer.joinExcludeContainers via TermSearch (ReferenceContainer.java:310,
 *    TermSearch.java:42-70): writes the joined container's rows (sorted) to rows_out. */
int yrwi_join_exclude(yrwi_ctx* ctx, const uint8_t* incl, int32_t nincl, const uint8_t* excl,
                      int32_t nexcl, int32_t max_distance, int64_t now_ms, uint8_t* rows_out,
                      int64_t cap_rows, int64_t* m);
/* == ReferenceOrder.normalizeWith + cardinal (ReferenceOrder.java:70,223) on one
 *    container (rows sorted by url hash), with settled min/max: score_out[i] =
 *    cardinal(row i). */
/* TermSearch(index, include, exclude, urlselection, ...).joined() for one query
 * descriptor (the urlselection of yrwi_query_desc honoured; k, profile, language
 * and filter unused): the joined and excluded container's rows, as
 * yrwi_join_exclude writes them. */
int yrwi_term_search(yrwi_ctx* ctx, const yrwi_query_desc* q, uint8_t* rows40_out, int64_t cap_rows, int64_t* m);
/* TermSearch.joined() of nq descriptors in one pass: the containers are planned and joined
 * together (as yrwi_query_batch joins a batch), the rows an exclusion removes are dropped on the
 * device, and what remains lands in rows40_out as one packed image.  row_off[0] = 0, the
 * offsets never decrease, and the rows of query i are rows40_out + 40 row_off[i] up to
 * row_off[i + 1]: byte for byte what yrwi_term_search(ctx, q + i, ...) writes for that
 * descriptor (one include term: the rows as stored; two or more: the joined record re-encoded
 * with that descriptor's own now_ms; exclusions, max_distance and urlselection honoured; k,
 * profile, language and filter unused).  An absent include term, an empty join or a fully
 * excluded container is an empty range, not an error; identical descriptors each get their
 * own range.
 *   Capacity: rows40_out == NULL only counts (cap_rows is ignored; row_off and st are filled;
 * returns 0).  Otherwise, when row_off[nq] > cap_rows the call returns YRWI_E_ARG with row_off
 * filled completely -- row_off[nq] is the capacity a retry needs -- and no byte of rows40_out
 * written: the pack kernel compares the total with cap_rows on the device before it stores a
 * row.  An upper bound that needs no extra pass: the sum over the queries of the smallest
 * include list (yrwi_list_size) -- a conjunction is no longer than its shortest list.
 *   Errors: planning errors (YRWI_E_HASH, the YRWI_E_UNSUPPORTED urlselection cases of
 * yrwi_query_desc, YRWI_E_ARG, YRWI_E_NOMEM) return before anything is written -- row_off and
 * rows40_out untouched -- and yrwi_last_error starts with "query <index>: ".  nq == 0 returns
 * 0 with row_off[0] = 0; nq < 0, or a NULL q or row_off with nq > 0, returns YRWI_E_ARG.  A
 * context of a shard group (world > 1) returns YRWI_E_UNSUPPORTED, as yrwi_event_add_local.
 * Waits for the batches in flight and changes nothing in the context; scratch comes from
 * lane 0's arena (no device allocation once it has its size).  st may be NULL.
 *   Where the rows go: rows40_out from yrwi_host_alloc and 8-byte aligned is written by the
 * pack kernel directly (st->direct = 1), as yrwi_dht_select and the hit rows of
 * yrwi_query_batch_rows are.  Any other buffer: the rows are packed in device scratch and leave
 * with one copy of exactly 40 row_off[nq] bytes (direct = 0).  Either way no row crosses PCIe
 * twice and an excluded row never crosses it.
 *   Shape of the call: after the join phase one upload, three kernels (k_local_count,
 * k_tsb_scan, k_tsb_pack) and the readback of the nq + 1 offsets -- launches_tail = 5 and one
 * host wait on the direct path; 6 and two waits on the pageable one (the copy is sized by the
 * total, so it follows the first wait).  Neither depends on nq or on the list lengths, nor do
 * the join phase's own waits (it writes its tile-group tables on the device, as for
 * yrwi_event_add_local).  A call whose containers are all empty before the exclusion enqueues
 * nothing after the join phase. */
typedef struct yrwi_tsb_stats {
  int64_t rows_joined, rows_out;   /* before / after exclusion, summed over the call (a chained fold excludes
                                      within its join: those rows are gone from rows_joined too) */
  int64_t bytes_h2d, bytes_d2h;    /* everything the call moved over PCIe */
  int32_t launches_tail;           /* launches, copies, memsets enqueued after the join phase */
  int32_t syncs;                   /* host waits on the device in the whole call */
  int32_t direct;                  /* 1: rows were stored straight into rows40_out */
  int64_t device_allocs;           /* yrwi_realloc_events of the call */
  int64_t t_pack_ns, t_total_ns;   /* HIP events around the pack launches; wall time */
} yrwi_tsb_stats;
int yrwi_term_search_batch(yrwi_ctx* ctx, const yrwi_query_desc* q, int32_t nq, uint8_t* rows40_out,
                           int64_t cap_rows, int64_t* row_off /* nq + 1 */, yrwi_tsb_stats* st);
/* Host facets of a query batch: per descriptor the hosts of its joined container and how many
 * postings each has -- the per-host score map a search event keeps for its "results by domain"
 * navigator (UNVERIFIED against a reference line: the reference counts hosts per search event
 * while results arrive and has no batch method for this).  Defined through this header: let R_i
 * be the rows yrwi_term_search_batch returns for descriptor i (exclusions, max_distance,
 * urlselection and now_ms honoured; k, profile, language and filter unused).  R_i is grouped by
 * host hash, the url-hash characters 6..11 (as yrwi_filter.sitehash).  nrows[i] = |R_i|,
 * nhosts[i] = its distinct hosts.  The hosts of query i are put in `order` and the first
 * min(nhosts[i], max_hosts) of them (max_hosts == 0: all) are written at index host_off[i] up to
 * host_off[i + 1]: six characters into hosts6_out, the host's postings in R_i into counts_out
 * and, when urls12_out is given, the smallest url hash of that host in R_i (a host name can
 * only be resolved through a url).  host_off[0] = 0; an empty R_i (an absent include term, an
 * empty join, a fully excluded container) is an empty range, not an error; identical
 * descriptors each get their own range; a host of several queries is counted per query.
 *   Capacity: hosts6_out == NULL && counts_out == NULL only counts (host_off, nhosts, nrows and
 * st are filled; the total is not compared with cap; urls12_out must be NULL too).  Otherwise both are given
 * and hold cap entries each (urls12_out 12 cap bytes); when host_off[nq] > cap the call returns
 * YRWI_E_ARG with host_off, nhosts and nrows filled and no byte of the three buffers written.
 *   Errors: planning errors return before anything is written and yrwi_last_error starts with
 * "query <index>: ".  An order outside YRWI_FACETS_BY_*, max_hosts < 0, cap < 0, nq < 0, a NULL q
 * or host_off with nq > 0, or only one of hosts6_out / counts_out: YRWI_E_ARG.  nq == 0 returns 0
 * with host_off[0] = 0; nq > 2^27 or 2^31 container rows in one call: YRWI_E_LIMIT.  A context
 * of a shard group (world > 1): YRWI_E_UNSUPPORTED, as yrwi_term_search_batch.  Waits for the
 * batches in flight and changes nothing in the context -- the dense host ids of the authority
 * path are neither needed nor built; scratch comes from lane 0's arena.  nhosts, nrows and st
 * may be NULL.
 *   Shape of the call: after the join phase one upload, the three kernels of the counting
 * yrwi_term_search_batch (the kept rows per query), seven launches of the group-by
 * (k_facet_keys, sort, k_facet_flag, scan, k_facet_runs, k_facet_query, scan) and ONE readback
 * of 3 nq + 2 words (host_off, nhosts, the kept-row offsets): launches_tail = 12 and one host
 * wait for a counting call, for one whose total exceeds cap and for one that has no host to
 * write.  A call that writes adds k_facet_pack and two copies (three with urls12_out), sized by
 * the total and so behind the first wait, and YRWI_FACETS_BY_COUNT two more launches (count
 * keys, sort) in front of them:
 *     launches_tail = 15 + (urls12_out ? 1 : 0) + (BY_COUNT ? 2 : 0), syncs = 2.
 * Neither depends on nq, on the lists or on their lengths.  A call whose containers are all
 * empty before the exclusion enqueues nothing after the join phase.  bytes_d2h = 8 (3 nq + 2)
 * + 14 hosts_out (26 hosts_out with urls12_out); a urlselection's planning reads its url ids
 * back besides. */
#define YRWI_FACETS_BY_HOST  0   /* ascending host hash (36-bit key order) */
#define YRWI_FACETS_BY_COUNT 1   /* postings descending; equal counts by ascending host hash */
typedef struct yrwi_facet_stats {
  int64_t rows_joined, rows_kept;  /* as yrwi_tsb_stats.rows_joined / rows_out */
  int64_t hosts, hosts_out;        /* sum over the queries of distinct hosts / of hosts written (host_off[nq]) */
  int64_t bytes_h2d, bytes_d2h;    /* everything the call moved over PCIe */
  int32_t launches_tail, syncs;    /* launches and copies enqueued, and host waits, after the join phase */
  int64_t device_allocs;           /* yrwi_realloc_events of the call */
  int64_t t_group_ns, t_total_ns;  /* HIP events around key, sort, heads, order, pack; wall time */
} yrwi_facet_stats;
int yrwi_host_facets_batch(yrwi_ctx* ctx, const yrwi_query_desc* q, int32_t nq, int32_t order, int32_t max_hosts,
                           uint8_t* hosts6_out, int64_t* counts_out, uint8_t* urls12_out /* may be NULL */,
                           int64_t cap, int64_t* host_off /* nq + 1 */, int64_t* nhosts /* nq, may be NULL */,
                           int64_t* nrows /* nq, may be NULL */, yrwi_facet_stats* st);
int yrwi_normalize_score(yrwi_ctx* ctx, const uint8_t* rows40, int64_t m, const yrwi_profile* prof,
                         const char* language, int64_t now_ms, int64_t* score_out);

#ifdef __cplusplus
}
#endif
#endif /* YRWI_H */
