// GpuRWI.java -- JNI binding of libyrwi (include/yrwi.h) for YaCy.
//
// UNVERIFIED: this image has no JDK (no javac, no jni.h), so this file and
// java/jni/yrwi_jni.c are shipped as the binding a YaCy maintainer would add;
// they have not been compiled here.  See INTEGRATION.md.
//
// Drop-in points (paths relative to source/net/yacy):
//   kelondro/rwi/TermSearch.java:42-70         -> GpuRWI.listSizes(...) + joinExclude(...) / termSearch(...) (GpuTermSearch)
//   kelondro/rwi/AbstractIndex.java:116        -> GpuRWI.getList(...) (TermSearch.inclusion, on demand)
//   kelondro/rwi/ReferenceContainer.java:310   -> GpuRWI.joinExclude(...)
//   search/ranking/ReferenceOrder.java:70,223  -> GpuRWI.eventOrder(...) (GpuReferenceOrder: one event per SearchEvent)
//   search/query/SearchEvent.java:612-631      -> GpuRWI.query(...) (whole local RWI path)
//   search/query/SearchEvent.java:736-806,1297 -> GpuRWI.queryFiltered(...) (constraints, doubledom)
//   search/query/SearchEvent.java:612-631,1297 -> GpuRWI.queryRows(...) (the hits with their joined postings: rwiStack elements)
//   search/query/SearchEvent.java:612-631,651  -> GpuRWI.eventAddLocal(...) (the local container into a GpuRWIStack event, device to device)
//   kelondro/rwi/IndexCell.java:353-386        -> GpuRWI.loadHeaps(...) (BLOB heaps into HBM)
//   kelondro/rwi/IndexCell.java:131-166        -> GpuRWI.dumpHeap(...) (the FlushThread dump: HBM into a BLOB heap)
//   peers/Dispatcher.selectContainersEnqueueToBuffer -> GpuRWI.dhtSelect(...) (select, remove and split containers for the DHT)
//
// Java level: 1.8, YaCy's own (build.properties javacSource/javacTarget, pom.xml
// maven.compiler.source/target).  No API newer than Java 8 is used here or in the
// other drop-ins (tests/test_java_sequence.py scans java/ for them).
package net.yacy.kelondro.rwi;

import java.lang.ref.PhantomReference;
import java.lang.ref.Reference;
import java.lang.ref.ReferenceQueue;
import java.util.ArrayList;
import java.util.Collections;
import java.util.Set;
import java.util.concurrent.ConcurrentHashMap;

public final class GpuRWI implements AutoCloseable {

    // A libyrwi context is not thread-safe (include/yrwi.h): every call on it is
    // synchronized on this object.  YaCy reaches one GpuRWI from the search threads,
    // the remote-peer (Protocol) threads and the result workers (authority()).

    static { System.loadLibrary("yrwi_jni"); }  // links libyrwi.so

    private long ctx;  // yrwi_ctx*

    /**
     * The release of one search event (GpuReferenceOrder, GpuRWIStack), Java 8 style:
     * a phantom reference to the object that owns the event.  The owner's close()
     * calls release(); an owner dropped without close() is released by this
     * context's reaper thread once the collector has enqueued the reference
     * (java.lang.ref.Cleaner does the same from Java 9 on, which YaCy's 1.8 build
     * does not have).  release() runs at most once.
     */
    public static final class EventHandle extends PhantomReference<Object> {
        private final GpuRWI gpu;
        private long event;

        EventHandle(final Object owner, final GpuRWI gpu, final long event, final ReferenceQueue<Object> q) {
            super(owner, q);
            this.gpu = gpu;
            this.event = event;
        }

        public void release() {
            final long e;
            synchronized (this) { e = this.event; this.event = 0; }
            if (e == 0) return;
            this.gpu.handles.remove(this);
            this.gpu.eventClose(e);
        }
    }

    private final ReferenceQueue<Object> unreachable = new ReferenceQueue<Object>();
    // the handles must stay strongly reachable until released, or they are collected themselves
    private final Set<EventHandle> handles = Collections.newSetFromMap(new ConcurrentHashMap<EventHandle, Boolean>());
    private final Thread reaper;

    public GpuRWI(final int device) {
        this.ctx = open(device);
        if (this.ctx == 0) throw new IllegalStateException("yrwi_open failed");
        final ReferenceQueue<Object> q = this.unreachable;
        this.reaper = new Thread(new Runnable() {
            @Override
            public void run() {
                while (true) {
                    final Reference<?> r;
                    try { r = q.remove(); } catch (final InterruptedException e) { return; }
                    if (r instanceof EventHandle) ((EventHandle) r).release();
                }
            }
        }, "GpuRWI event reaper");
        this.reaper.setDaemon(true);
        this.reaper.start();
    }

    /** Registers `event` for release when `owner` becomes unreachable (or at close()). */
    public EventHandle track(final Object owner, final long event) {
        final EventHandle h = new EventHandle(owner, this, event, this.unreachable);
        this.handles.add(h);
        return h;
    }

    /** IndexCell.add for a whole container: the RowSet chunkcache bytes (n * 40, sorted). */
    public synchronized void putList(final byte[] termHash, final byte[] chunkcache, final int n) {
        check(putList(this.ctx, termHash, chunkcache, n, 1));
    }

    /** Policies of addPostings (YRWI_ADD_*): which of a (term, url) pair's candidates stays. */
    public static final int ADD_REPLACE = 0;  // RowSet.put: IndexCell.add(termHash, entry), ReferenceContainerCache.add
    public static final int ADD_KEEP = 1;     // RowSet.mergeEnum: IndexCell.add(container) merged below what is stored
    public static final int ADD_RECENT = 2;   // ReferenceContainer.putAllRecent (DHT transfers)

    /** IndexCell.add in bulk (yrwi_add_postings): posting i is rows[40 i, 40 i + 40) for the list of the
     *  term hash terms[12 i, 12 i + 12), in any order; only the batch crosses to the device.  Returns
     *  {terms, newTerms, emptiedTerms, added, replaced, dropped, removed, launches, syncs}. */
    public synchronized long[] addPostings(final byte[] terms, final byte[] rows, final int n, final int policy) {
        final long[] st = addPostings(this.ctx, terms, rows, n, policy);
        if (st == null) throw new IllegalStateException("yrwi_add_postings failed");
        return st;
    }

    /** IndexCell.remove(termHash, urlHashes) for every term of `terms`; terms == null or empty: every
     *  list (Segment.removeAllUrlReferences without the document's words).  Returns the statistics
     *  of addPostings (removed = rows removed). */
    public synchronized long[] removePostings(final byte[][] terms, final byte[][] urls) {
        final int nterms = terms == null ? 0 : terms.length;
        final long[] st = removePostings(this.ctx, nterms == 0 ? new byte[0] : flatten(terms), nterms,
                                         flatten(urls), urls.length);
        if (st == null) throw new IllegalStateException("yrwi_remove_postings failed");
        return st;
    }

    /** Removes every posting whose url hash carries one of the host hashes (6 bytes each: url-hash
     *  characters 6..11, as queryFiltered's sitehash) from the lists of `terms`; terms == null or empty:
     *  from every list (yrwi_remove_hosts).  The hosts' url hashes are found on the device: no list
     *  crosses to the host.  Returns the statistics of removePostings.  Uncompiled like the rest of
     *  this class (see the head of the file). */
    public synchronized long[] removeHosts(final byte[][] terms, final byte[][] hosts) {
        final int nterms = terms == null ? 0 : terms.length;
        final long[] st = removeHosts(this.ctx, nterms == 0 ? new byte[0] : flatten(terms), nterms,
                                      flattenN(hosts, 6), hosts.length);
        if (st == null) throw new IllegalStateException("yrwi_remove_hosts failed");
        return st;
    }

    /** What removeHosts(terms, hosts) would remove, the index unchanged (yrwi_count_hosts):
     *  long[hosts.length + 1] = the postings of every host in the selected lists (a host given twice
     *  gets its count twice), then the number of selected lists that hold at least one of them. */
    public synchronized long[] countHosts(final byte[][] terms, final byte[][] hosts) {
        final int nterms = terms == null ? 0 : terms.length;
        final long[] counts = countHosts(this.ctx, nterms == 0 ? new byte[0] : flatten(terms), nterms,
                                         flattenN(hosts, 6), hosts.length);
        if (counts == null) throw new IllegalStateException("yrwi_count_hosts failed");
        return counts;
    }

    /** Orders of urlReferences (YRWI_REFS_BY_*). */
    public static final int REFS_BY_TERM = 0;  // ascending term hash, the references of one list by ascending url hash
    public static final int REFS_BY_URL = 1;   // ascending url hash, the references of one url by ascending term hash

    /** What urlReferences returns: counts[i] = the references of urls[i] (a url given twice gets its count
     *  twice); with fetch, reference r is rows[r] (the 40-byte row as stored) in the list of terms[r], in the
     *  order asked for; without, terms and rows are null.  stats = {lists, postings, urls, urlsFound, refs,
     *  listsHit, listsCovered, path, direct, launches, syncs, bytesH2d, bytesD2h, tFindNs, tTotalNs}
     *  (yrwi_ref_stats): refs, listsHit and listsCovered are removed, terms and emptiedTerms of
     *  removePostings(terms, urls). */
    public static final class UrlReferences {
        public final long[] counts;
        public final byte[][] terms;
        public final byte[][] rows;
        public final long[] stats;
        UrlReferences(final long[] counts, final byte[][] terms, final byte[][] rows, final long[] stats) {
            this.counts = counts;
            this.terms = terms;
            this.rows = rows;
            this.stats = stats;
        }
    }

    /** What removePostings(terms, urls) would remove, the index unchanged (yrwi_url_references): which
     *  words index these urls, how many references each url has and, with fetch, the rows themselves (to
     *  move, re-host, re-send or re-add them).  terms == null or empty: every list.  The references are
     *  found on the device and only they cross to the host.  No reference method stands behind this:
     *  Segment.removeAllUrlReferences re-loads and re-parses the document to learn its words.  A first
     *  call counts, a second one fetches into arrays of that size.  Uncompiled like the rest of this
     *  class (see the head of the file). */
    public synchronized UrlReferences urlReferences(final byte[][] terms, final byte[][] urls, final int order,
                                                    final boolean fetch) {
        final int nterms = terms == null ? 0 : terms.length;
        final byte[] t = nterms == 0 ? new byte[0] : flatten(terms);
        final byte[] u = flatten(urls);
        long[] r = urlReferences(this.ctx, t, nterms, u, urls.length, order, 0L, null, null);
        if (r == null) throw new IllegalStateException("yrwi_url_references failed");
        final long refs = r[4];
        byte[][] outTerms = null;
        byte[][] outRows = null;
        if (fetch) {
            if (40L * refs > Integer.MAX_VALUE) throw new IllegalArgumentException("more references than a byte[] holds: name fewer urls");
            final int n = (int) refs;
            final byte[] t12 = new byte[12 * n];
            final byte[] r40 = new byte[40 * n];
            if (n > 0) {
                r = urlReferences(this.ctx, t, nterms, u, urls.length, order, refs, t12, r40);
                if (r == null || r[15] != 0 || r[4] != refs) throw new IllegalStateException("yrwi_url_references failed");
            }
            outTerms = new byte[n][];
            outRows = new byte[n][];
            for (int i = 0; i < n; i++) {
                outTerms[i] = java.util.Arrays.copyOfRange(t12, 12 * i, 12 * i + 12);
                outRows[i] = java.util.Arrays.copyOfRange(r40, 40 * i, 40 * i + 40);
            }
        }
        return new UrlReferences(java.util.Arrays.copyOfRange(r, 16, 16 + urls.length), outTerms, outRows,
                                 java.util.Arrays.copyOfRange(r, 0, 15));
    }

    /** Orders of hostCensus (YRWI_CENSUS_BY_*). */
    public static final int CENSUS_BY_HOST = 0;   // ascending host hash (Base64Order)
    public static final int CENSUS_BY_COUNT = 1;  // postings descending, equal counts by ascending host hash

    /** What hostCensus returns: hosts[i] (6 bytes, url-hash characters 6..11) has counts[i] postings in
     *  the selected lists; stats = {lists, postings, hosts, hostsPassing, tableSlots, passes, ldsBypass,
     *  launches, syncs, tCountNs, tTotalNs} (yrwi_census_stats). */
    public static final class HostCensus {
        public final byte[][] hosts;
        public final long[] counts;
        public final long[] stats;
        HostCensus(final byte[][] hosts, final long[] counts, final long[] stats) {
            this.hosts = hosts;
            this.counts = counts;
            this.stats = stats;
        }
    }

    /** Which hosts have postings in the lists of `terms` (terms == null or empty: in every list) and how
     *  many each (yrwi_host_census): the hosts with at least minPostings postings in `order`, the first
     *  `top` of them, or all of them with top &lt; 0 (a first call asks how many pass).  The counts are
     *  those countHosts gives for the same hosts and terms; no list crosses to the host.  The front end
     *  of removeHosts: the index-wide form of the per-container host counts of ReferenceOrder.doms. */
    public synchronized HostCensus hostCensus(final byte[][] terms, final int order, final long minPostings,
                                              final long top) {
        final int nterms = terms == null ? 0 : terms.length;
        final byte[] t = nterms == 0 ? new byte[0] : flatten(terms);
        long cap = top;
        if (cap < 0) {
            final long[] r = hostCensus(this.ctx, t, nterms, order, minPostings, 0L, new byte[0]);
            if (r == null) throw new IllegalStateException("yrwi_host_census failed");
            cap = r[4];  // hostsPassing
        }
        if (6L * cap > Integer.MAX_VALUE) throw new IllegalArgumentException("more hosts than a byte[] holds: give top");
        final byte[] h6 = new byte[(int) (6L * cap)];
        final long[] r = hostCensus(this.ctx, t, nterms, order, minPostings, cap, h6);
        if (r == null) throw new IllegalStateException("yrwi_host_census failed");
        final int n = (int) r[0];
        final byte[][] hosts = new byte[n][];
        final long[] counts = new long[n];
        for (int i = 0; i < n; i++) {
            hosts[i] = java.util.Arrays.copyOfRange(h6, 6 * i, 6 * i + 6);
            counts[i] = r[12 + i];
        }
        return new HostCensus(hosts, counts, java.util.Arrays.copyOfRange(r, 1, 12));
    }

    /** Entries of the day histogram of retentionCount: one per value of the 16-bit lastModified cell. */
    public static final int RETENTION_DAYS = 65536;

    /** What retain(terms, minDay, maxRefs) would remove, the index unchanged (yrwi_retention_count):
     *  long[15] = {lists, postings, removedAge, removedCap, listsAge, listsCap, emptiedTerms, dayMin,
     *  dayMax, launches, syncs, tMarkNs, tSelectNs, tTotalNs, histBypass} (yrwi_retention_stats), and with
     *  hist the RETENTION_DAYS entries of the histogram of the selected rows' lastModified days after them
     *  (counted before any rule: what a caller picks the minDay from that reaches a target size). */
    public synchronized long[] retentionCount(final byte[][] terms, final int minDay, final long maxRefs,
                                              final boolean hist) {
        final int nterms = terms == null ? 0 : terms.length;
        final long[] st = retentionCount(this.ctx, nterms == 0 ? new byte[0] : flatten(terms), nterms, minDay,
                                         maxRefs, hist ? 1 : 0);
        if (st == null) throw new IllegalStateException("yrwi_retention_count failed");
        return st;
    }

    /** Retention on the device (yrwi_retain): from the lists of `terms` (terms == null or empty: from every
     *  list) every posting whose lastModified day is below minDay goes (0: no age rule), then a list that
     *  still has more than maxRefs rows (0: no cap) keeps its maxRefs newest, equal days at the cut in
     *  url-hash order.  No list crosses to the host.  Returns long[24]: the statistics of removePostings,
     *  then those of retentionCount.  The rules are this project's: the reference has no such method. */
    public synchronized long[] retain(final byte[][] terms, final int minDay, final long maxRefs) {
        final int nterms = terms == null ? 0 : terms.length;
        final long[] st = retain(this.ctx, nterms == 0 ? new byte[0] : flatten(terms), nterms, minDay, maxRefs);
        if (st == null) throw new IllegalStateException("yrwi_retain failed");
        return st;
    }

    /** Index.size(termHash) of each term on the GPU index (yrwi_list_size; 0: no list). */
    public synchronized long[] listSizes(final byte[][] terms) {
        return listSizes(this.ctx, flatten(terms), terms.length);
    }

    /** Index.get(termHash) off the query path (yrwi_get_list): the list's sorted rows (n * 40 bytes). */
    public synchronized byte[] getList(final byte[] term) {
        final byte[] rows = getList(this.ctx, term);
        if (rows == null) throw new IllegalStateException("yrwi_get_list failed");
        return rows;
    }

    /** TermSearch + joinExcludeContainers: returns the joined container's rows (m * 40 bytes). */
    public synchronized byte[] joinExclude(final byte[][] include, final byte[][] exclude, final int maxDistance,
                              final long nowMillis) {
        return joinExclude(this.ctx, flatten(include), include.length, flatten(exclude), exclude.length,
                           maxDistance, nowMillis);
    }

    /** TermSearch(..., urlselection, ...).joined(): every include and exclude list restricted
     *  to the url selection (url hashes) before the conjunction, as
     *  ReferenceContainerCache.get(key, urlselection) restricts it (yrwi_term_search). */
    public synchronized byte[] termSearch(final byte[][] include, final byte[][] exclude, final byte[][] urlselection,
                             final int maxDistance, final long nowMillis) {
        final byte[] rows = termSearch(this.ctx, flatten(include), include.length, flatten(exclude), exclude.length,
                                       urlselection == null ? null : flatten(urlselection),
                                       urlselection == null ? 0 : urlselection.length, maxDistance, nowMillis);
        if (rows == null) throw new IllegalStateException("yrwi_term_search failed");
        return rows;
    }

    /** TermSearch.joined() of many queries in one pass (yrwi_term_search_batch): one planning
     *  and join pass for all of them, the excluded rows dropped on the device.  Query i has the
     *  term hashes include[i] / exclude[i], the url selection urlselection[i] (the array or an
     *  entry may be null: none), maxDistance[i] and nowMillis[i].  Returns the packed rows of
     *  all queries and fills rowOff (length &gt;= include.length + 1): query i owns the rows
     *  rowOff[i] .. rowOff[i + 1], 40 bytes each, byte for byte what termSearch / joinExclude
     *  return for it. */
    public synchronized byte[] termSearchBatch(final byte[][][] include, final byte[][][] exclude,
                                  final byte[][][] urlselection, final int[] maxDistance, final long[] nowMillis,
                                  final long[] rowOff) {
        final int nq = include.length;
        final int[] ni = new int[nq], ne = new int[nq], ns = new int[nq];
        for (int i = 0; i < nq; i++) {
            ni[i] = include[i].length;
            ne[i] = exclude[i] == null ? 0 : exclude[i].length;
            ns[i] = urlselection == null || urlselection[i] == null ? 0 : urlselection[i].length;
        }
        final byte[] rows = termSearchBatch(this.ctx, nq, flatten3(include), ni, flatten3(exclude), ne,
                                            urlselection == null ? null : flatten3(urlselection),
                                            urlselection == null ? null : ns, maxDistance, nowMillis, rowOff);
        if (rows == null) throw new IllegalStateException("yrwi_term_search_batch failed");
        return rows;
    }

    /** yrwi_host_facets_batch orders. */
    public static final int FACETS_BY_HOST = 0, FACETS_BY_COUNT = 1;

    /** What hostFacets returns: per query the hosts of its joined container.  Query i owns the
     *  entries hostOff[i] .. hostOff[i + 1] of hosts (6 bytes each), counts and urls (12 bytes
     *  each, or null when not asked for). */
    public static final class HostFacets {
        public final byte[] hosts;    // host hashes (url-hash characters 6..11), 6 bytes each
        public final long[] counts;   // postings of each host in its query's container
        public final byte[] urls;     // the smallest url hash of each host in that container, or null
        public final long[] hostOff;  // nq + 1 entry offsets
        public final long[] nhosts;   // distinct hosts of every query (before the maxHosts cut)
        public final long[] nrows;    // rows of every query's container
        /** the fields of yrwi_facet_stats in their order */
        public final long[] stats;

        HostFacets(final byte[] hosts, final long[] counts, final byte[] urls, final long[] hostOff,
                   final long[] nhosts, final long[] nrows, final long[] stats) {
            this.hosts = hosts;
            this.counts = counts;
            this.urls = urls;
            this.hostOff = hostOff;
            this.nhosts = nhosts;
            this.nrows = nrows;
            this.stats = stats;
        }

        /** the host hash of entry j */
        public byte[] host(final int j) {
            return java.util.Arrays.copyOfRange(this.hosts, 6 * j, 6 * j + 6);
        }
    }

    /** The "results by domain" navigator of many queries in one pass (yrwi_host_facets_batch):
     *  per query the hosts of its joined container (the rows termSearchBatch returns for it),
     *  the postings of each and, with wantUrls, each host's smallest url hash -- a host name is
     *  resolved through a url.  order: FACETS_BY_HOST or FACETS_BY_COUNT (postings descending,
     *  equal counts by ascending host hash); maxHosts: the most hosts per query, 0: all.  The
     *  queries are given as for termSearchBatch.  Only the triples leave the device. */
    public synchronized HostFacets hostFacets(final byte[][][] include, final byte[][][] exclude,
                                              final byte[][][] urlselection, final int[] maxDistance,
                                              final long[] nowMillis, final int order, final int maxHosts,
                                              final boolean wantUrls) {
        final int nq = include.length;
        final int[] ni = new int[nq], ne = new int[nq], ns = new int[nq];
        for (int i = 0; i < nq; i++) {
            ni[i] = include[i].length;
            ne[i] = exclude[i] == null ? 0 : exclude[i].length;
            ns[i] = urlselection == null || urlselection[i] == null ? 0 : urlselection[i].length;
        }
        final long[] hostOff = new long[nq + 1], nhosts = new long[nq], nrows = new long[nq], stats = new long[11];
        final Object[] r = hostFacets(this.ctx, nq, flatten3(include), ni, flatten3(exclude), ne,
                                      urlselection == null ? null : flatten3(urlselection),
                                      urlselection == null ? null : ns, maxDistance, nowMillis, order, maxHosts,
                                      wantUrls, hostOff, nhosts, nrows, stats);
        if (r == null) throw new IllegalStateException("yrwi_host_facets_batch failed");
        return new HostFacets((byte[]) r[0], (long[]) r[1], (byte[]) r[2], hostOff, nhosts, nrows, stats);
    }

    /** joinExclude into a caller-owned direct buffer (ByteBuffer.allocateDirect, reused
     *  across queries): no copy of the joined container through a Java array.  Returns
     *  the number of 40-byte rows written; throws when the container does not fit. */
    public synchronized long joinExcludeInto(final byte[][] include, final byte[][] exclude, final int maxDistance,
                                final long nowMillis, final java.nio.ByteBuffer out) {
        final long m = joinExcludeInto(this.ctx, flatten(include), include.length, flatten(exclude), exclude.length,
                                       maxDistance, nowMillis, out);
        if (m < 0) check((int) m);
        return m;
    }

    /** ReferenceOrder.normalizeWith + cardinal with settled min/max: one score per row. */
    public synchronized long[] normalizeScore(final byte[] rows, final int m, final int[] profile32, final String language,
                                 final long nowMillis) {
        return normalizeScore(this.ctx, rows, m, profile32, language, nowMillis);
    }

    /** SearchEvent local RWI path: top-k (urlhash, cardinal) of one query. Output: k * 24 bytes
     *  (12-byte url hash, int32 ByteArray.hashCode, int64 score), little endian. */
    public synchronized byte[] query(final byte[][] include, final byte[][] exclude, final int maxDistance, final int k,
                        final int[] profile32, final String language, final long nowMillis) {
        return query(this.ctx, flatten(include), include.length, flatten(exclude), exclude.length, maxDistance, k,
                     profile32, language, nowMillis, null);
    }

    /** query(...) with the call's yrwi_stats (17 longs, order in yrwi_jni.c stats_out):
     *  postings in, joined rows, algorithmic bytes, per-phase device times, launches. */
    public synchronized byte[] query(final byte[][] include, final byte[][] exclude, final int maxDistance, final int k,
                        final int[] profile32, final String language, final long nowMillis, final long[] stats) {
        return query(this.ctx, flatten(include), include.length, flatten(exclude), exclude.length, maxDistance, k,
                     profile32, language, nowMillis, stats);
    }

    /** IndexCell's BLOB heaps (text.index.*.blob) into the GPU index; lists already
     *  present act as the RAM cache.  Returns {files, records, free, badKeys, terms,
     *  postings, droppedTerms}. */
    public synchronized long[] loadHeaps(final String[] heapFiles, final boolean orderByFileName) {
        return loadHeaps(this.ctx, heapFiles, orderByFileName ? 1 : 0);
    }

    /** The FlushThread dump of IndexCell (IndexCell.java:131-166 through HeapWriter.add and
     *  RowCollection.exportCollection; yrwi_dump_heap): the lists of `terms`, or with terms == null or
     *  empty every list, written to one BLOB heap file in term-hash order; the file appears under
     *  `path` only when complete (written to path + ".prt", then renamed).  Name it
     *  prefix.yyyyMMddHHmmssSSS.blob for ArrayStack and loadHeaps(..., orderByFileName).  nowMs: the
     *  time for the export header's day cells (0: now).  Returns {terms, postings, bytes, windows,
     *  launches, syncs, packNanos, totalNanos}. */
    public synchronized long[] dumpHeap(final String path, final byte[][] terms, final long nowMs) {
        final int nterms = terms == null ? 0 : terms.length;
        final long[] st = dumpHeap(this.ctx, path, nterms == 0 ? new byte[0] : flatten(terms), nterms, nowMs);
        if (st == null) throw new IllegalStateException("yrwi_dump_heap failed");
        return st;
    }

    /** yrwi_dht_select flags. */
    public static final int DHT_ROT = 1, DHT_REMOVE = 2, DHT_SKIP_PRIVATE = 4, DHT_COUNT_ONLY = 8;

    /** What dhtSelect returns: the containers Dispatcher.selectContainers takes, split as
     *  Dispatcher.splitContainers splits them.  Cell (p, j) -- the postings of terms[j] that go to
     *  vertical partition p -- is rows[40 * partOff[p * T + j] .. 40 * partOff[p * T + j + 1]), T the
     *  number of terms, in url-hash order. */
    public static final class DhtSelection {
        public final byte[][] terms;   // T term hashes in selection order
        public final long[] partOff;   // 2^e * T + 1 row offsets, partition-major
        public final byte[] rows;      // every selected posting, 40 bytes each, cell after cell
        public final int partitions;   // 2^e
        /** {terms, postings, skippedPrivate, removed, wrapped, windows, launches, syncs, packNanos, totalNanos} */
        public final long[] stats;

        DhtSelection(final byte[][] terms, final long[] partOff, final byte[] rows, final int partitions,
                     final long[] stats) {
            this.terms = terms;
            this.partOff = partOff;
            this.rows = rows;
            this.partitions = partitions;
            this.stats = stats;
        }

        /** the postings of terms[j] for partition p, 40 bytes each */
        public byte[] cell(final int p, final int j) {
            final int c = p * this.terms.length + j;
            return java.util.Arrays.copyOfRange(this.rows, (int) (40 * this.partOff[c]), (int) (40 * this.partOff[c + 1]));
        }
    }

    /** The DHT send path, Dispatcher.selectContainersEnqueueToBuffer on the device (yrwi_dht_select):
     *  selectContainers from the first term >= start -- whole containers in term order while fewer
     *  than maxContainers are taken, fewer than maxRefs references, and the term is below limit (the
     *  first one whatever it is); with DHT_ROT on from the smallest term after the largest --, the
     *  split of each by Distribution.verticalDHTPosition into 2^partitionExponent partitions, and with
     *  DHT_REMOVE IndexCell.remove(termHash) of what was selected.  Transmission sends each
     *  partition's cells to its target peers; what could not be sent goes back through
     *  addPostings(..., ADD_KEEP).  DHT_COUNT_ONLY: only stats are filled. */
    public synchronized DhtSelection dhtSelect(final byte[] start, final byte[] limit, final int maxContainers,
                                               final long maxRefs, final int partitionExponent, final int flags) {
        final long[] stats = new long[10];
        final Object[] r = dhtSelect(this.ctx, start, limit, maxContainers, maxRefs, partitionExponent, flags, stats);
        if (r == null) throw new IllegalStateException("yrwi_dht_select failed");
        if ((flags & DHT_COUNT_ONLY) != 0) {
            return new DhtSelection(new byte[0][], new long[] {0L}, new byte[0], 1 << partitionExponent, stats);
        }
        final byte[] flat = (byte[]) r[0];
        final byte[][] terms = new byte[flat.length / 12][];
        for (int j = 0; j < terms.length; j++) terms[j] = java.util.Arrays.copyOfRange(flat, 12 * j, 12 * j + 12);
        return new DhtSelection(terms, (long[]) r[1], (byte[]) r[2], 1 << partitionExponent, stats);
    }

    /** query(...) under SearchEvent.addRWIs constraints (SearchEvent.java:736-806) and,
     *  with skipDoubleDom, in pullOneRWI order (:1297-1394).  flagCount (int[32] or null)
     *  receives SearchEvent.flagcount. */
    public synchronized byte[] queryFiltered(final byte[][] include, final byte[][] exclude, final int maxDistance, final int k,
                                final int[] profile32, final String language, final long nowMillis,
                                final byte[] constraint, final boolean allOfConstraint, final int contentdom,
                                final boolean strictContentDom, final String modifierLanguage, final byte[] sitehash,
                                final byte[] altSitehash, final byte[][] siteexcludes, final byte[][] urlhashes,
                                final boolean skipDoubleDom, final int[] flagCount) {
        return queryFiltered(this.ctx, flatten(include), include.length, flatten(exclude), exclude.length,
                             maxDistance, k, profile32, language, nowMillis, constraint, allOfConstraint, contentdom,
                             strictContentDom, modifierLanguage, sitehash, altSitehash, flattenN(siteexcludes, 6),
                             flattenN(urlhashes, 12), skipDoubleDom, flagCount);
    }

    /** The hits of queryFiltered(...) together with the joined posting of every hit
     *  (yrwi_query_rows): what SearchEvent.rwiStack holds and pullOneRWI hands to
     *  Fulltext.getMetadata (SearchEvent.java:1297-1394).  rows: one 40-byte WordReferenceRow
     *  per hit, in hit order -- the row TermSearch.joined() holds for the hit's url (one
     *  include word: the stored row; more: the joined posting as toRowEntry writes it). */
    public static final class HitsWithRows {
        public final byte[] hits;   // n * 24 bytes, as query()
        public final byte[] rows;   // n * 40 bytes
        HitsWithRows(final byte[] hits, final byte[] rows) {
            this.hits = hits;
            this.rows = rows;
        }
        public int size() {
            return this.hits.length / 24;
        }
        /** the 40 bytes of hit i's posting (new WordReferenceRow(urlEntryRow.newEntry(row(i)))) */
        public byte[] row(final int i) {
            final byte[] r = new byte[40];
            System.arraycopy(this.rows, 40 * i, r, 0, 40);
            return r;
        }
    }

    /** queryFiltered(...) returning the hits plus their rows in one call; the filter arguments
     *  may all be null / false / -1 (an unconstrained query).  A sharded context returns 40
     *  zero bytes for a hit whose url hash another rank owns (include/yrwi.h). */
    public synchronized HitsWithRows queryRows(final byte[][] include, final byte[][] exclude, final int maxDistance,
                                final int k, final int[] profile32, final String language, final long nowMillis,
                                final byte[] constraint, final boolean allOfConstraint, final int contentdom,
                                final boolean strictContentDom, final String modifierLanguage, final byte[] sitehash,
                                final byte[] altSitehash, final byte[][] siteexcludes, final byte[][] urlhashes,
                                final boolean skipDoubleDom, final int[] flagCount) {
        final byte[][] r = queryRows(this.ctx, flatten(include), include.length, flatten(exclude), exclude.length,
                                     maxDistance, k, profile32, language, nowMillis, constraint, allOfConstraint,
                                     contentdom, strictContentDom, modifierLanguage, sitehash, altSitehash,
                                     flattenN(siteexcludes, 6), flattenN(urlhashes, 12), skipDoubleDom, flagCount);
        if (r == null) throw new IllegalStateException("yrwi_query_rows failed");
        return new HitsWithRows(r[0], r[1]);
    }

    /** A SearchEvent's rwiStack on the GPU: open once per event, then addRWIs for the
     *  local container and every remote peer's container (Protocol.java:802); the
     *  result is the stack in rwiStack order (24-byte records as query()). */
    public synchronized long eventOpen(final int[] profile32, final String language, final long nowMillis, final int k,
                          final long maxPostings) {
        return eventOpen(this.ctx, profile32, language, nowMillis, k, maxPostings);
    }

    /** SearchEvent.addRWIs constraints of one event (SearchEvent.java:736-806), the
     *  fields of QueryParams queryFiltered takes; null arrays: no such constraint. */
    public static final class EventFilter {
        public byte[] constraint;          // Bitfield bytes (4) or null
        public boolean allOfConstraint;
        public int contentdom = -1;        // ContentDomain code, -1: ALL
        public boolean strictContentDom;
        public String modifierLanguage;    // QueryModifier.language or null
        public byte[] sitehash, altSitehash;  // 6-byte host hashes or null
        public byte[][] siteexcludes;      // 6-byte host hashes or null
        public byte[][] urlhashes;         // url hashes already in SearchEvent.urlhashes (doublecheck) or null
    }

    /** A full search event (url set, rwiStack, doubleDomCache) under constraints: GpuRWIStack. */
    public synchronized long eventOpenFiltered(final int[] profile32, final String language, final long nowMillis,
                                               final int k, final long maxPostings, final EventFilter f) {
        if (f == null) return eventOpen(this.ctx, profile32, language, nowMillis, k, maxPostings);
        return eventOpenFiltered(this.ctx, profile32, language, nowMillis, k, maxPostings, f.constraint,
                                 f.allOfConstraint, f.contentdom, f.strictContentDom, f.modifierLanguage, f.sitehash,
                                 f.altSitehash, flattenN(f.siteexcludes, 6), flattenN(f.urlhashes, 12));
    }

    /** (arrival, row) pairs of the postings the event's doublecheck admitted for n url
     *  hashes (12 bytes each): arrival 1 = the first addRWIs, 0 = seeded, -1 = absent. */
    public synchronized int[] eventSource(final long event, final byte[] urls, final int n) {
        final int[] s = eventSource(this.ctx, event, urls, n);
        if (s == null) throw new IllegalStateException("yrwi_event_source failed");
        return s;
    }

    /** SearchEvent.flagcount of an event (yrwi_event_result's info). */
    public synchronized int[] eventFlagCount(final long event) {
        final int[] fc = eventFlagCount(this.ctx, event);
        if (fc == null) throw new IllegalStateException("yrwi_event_result failed");
        return fc;
    }

    /** An event holding only a SearchEvent's ReferenceOrder (yrwi_event_open_order):
     *  eventOrder / eventAuthority only, the host table sized for maxHosts hosts; device
     *  memory comes from closed order-only events (no device-wide allocation per event). */
    public synchronized long eventOpenOrder(final int[] profile32, final String language, final long nowMillis,
                                            final long maxHosts) {
        return eventOpenOrder(this.ctx, profile32, language, nowMillis, maxHosts);
    }

    public synchronized void addRWIs(final long event, final byte[] containerRows, final int n, final boolean local) {
        check(eventAdd(this.ctx, event, containerRows, n, local));
    }

    /** addRWIs(termSearch.joined(), local = true) for an index that is this GpuRWI's
     *  (yrwi_event_add_local): the joined and excluded container of the terms arrives at
     *  the event without its rows leaving the device; urlselection as termSearch takes it,
     *  or null.  Returns the rows that arrived (0: an empty container, the event and its
     *  arrival numbering are unchanged).  Not on a shard of a sharded index. */
    public synchronized long eventAddLocal(final long event, final byte[][] include, final byte[][] exclude,
                                           final byte[][] urlselection, final int maxDistance, final long nowMillis) {
        final long m = eventAddLocal(this.ctx, event, flatten(include), include.length, flatten(exclude),
                                     exclude.length, urlselection == null ? null : flatten(urlselection),
                                     urlselection == null ? 0 : urlselection.length, maxDistance, nowMillis);
        if (m < 0) check((int) m);
        return m;
    }

    /** The rows the event retained from eventAddLocal arrivals for n url hashes (12 bytes each;
     *  yrwi_event_rows): n * 40 row bytes, then n found bytes -- 1 where the url's admitted
     *  posting arrived through eventAddLocal, 0 (and 40 zero bytes) where the url is not in the
     *  doublecheck set, was seeded, or came from an addRWIs arrival (the caller has those rows). */
    public synchronized byte[] eventRows(final long event, final byte[] urls, final int n) {
        final byte[] r = eventRows(this.ctx, event, urls, n);
        if (r == null) throw new IllegalStateException("yrwi_event_rows failed");
        return r;
    }

    /** ReferenceOrder.normalizeWith(container, local) + cardinal of every row, continuing
     *  the event's ReferenceOrder (yrwi_event_order): min/max, the max-distance fold and
     *  the host counts accumulate over every container given to the event; the scores
     *  are under the state after this one.  The event's stack is not touched. */
    public synchronized long[] eventOrder(final long event, final byte[] containerRows, final int n, final boolean local) {
        final long[] sc = eventOrder(this.ctx, event, containerRows, n, local);
        if (sc == null) throw new IllegalStateException("yrwi_event_order failed");
        return sc;
    }

    /** ReferenceOrder.authority(hostHash) against the event's accumulated host counts. */
    public synchronized int eventAuthority(final long event, final byte[] hostHash6) {
        final int[] a = eventAuthority(this.ctx, event, hostHash6, 1);
        if (a == null) throw new IllegalStateException("yrwi_event_authority failed");
        return a[0];
    }

    /** eventAuthority for n host hashes at once (6 bytes each, concatenated): one call. */
    public synchronized int[] eventAuthorities(final long event, final byte[] hostHashes6, final int n) {
        final int[] a = eventAuthority(this.ctx, event, hostHashes6, n);
        if (a == null) throw new IllegalStateException("yrwi_event_authority failed");
        return a;
    }

    public synchronized byte[] eventResult(final long event, final int maxn) {
        return eventResult(this.ctx, event, maxn);
    }

    /** SearchEvent.pullOneRWI(skipDoubleDom) up to maxn times (SearchEvent.java:1297-1394):
     *  yrwi_hit records (12-byte url hash, int hashCode, long score) in pull order;
     *  the entries leave the event's rwiStack, the doubleDomCache stays with the event. */
    public synchronized byte[] pullRWI(final long event, final boolean skipDoubleDom, final int maxn) {
        return eventPull(this.ctx, event, skipDoubleDom, maxn);
    }

    public synchronized void eventClose(final long event) {
        if (this.ctx != 0) eventClose(this.ctx, event);  // after close() the context freed it
    }

    /** WordReferenceFactory.compressIndex of each include word's list (search.java:264-281):
     *  one "{...}" per word; empty when a word has no list (searchConjunction is empty). */
    public synchronized String[] indexAbstracts(final byte[][] words, final long capacity) {
        return indexAbstracts(this.ctx, flatten(words), words.length, capacity);
    }

    /** ReferenceOrder.cardinal(URIMetadataNode) of packed yrwi_node records (60 bytes each). */
    public synchronized long[] scoreNodes(final byte[] nodes, final int n, final int[] profile32, final String language,
                             final int maxdomcount) {
        return scoreNodes(this.ctx, nodes, n, profile32, language, maxdomcount);
    }

    @Override
    public synchronized void close() {
        if (this.ctx == 0) return;
        this.reaper.interrupt();
        for (final EventHandle h : new ArrayList<EventHandle>(this.handles)) h.release();  // events before the context
        close(this.ctx);
        this.ctx = 0;
    }

    /** RankingProfile public coefficients in declaration order (RankingProfile.java:81-88). */
    public static int[] profile32(final net.yacy.search.ranking.RankingProfile p) {
        return new int[] {
            p.coeff_domlength, p.coeff_date, p.coeff_wordsintitle, p.coeff_wordsintext, p.coeff_phrasesintext,
            p.coeff_llocal, p.coeff_lother, p.coeff_urllength, p.coeff_urlcomps, p.coeff_hitcount,
            p.coeff_posintext, p.coeff_posofphrase, p.coeff_posinphrase, p.coeff_authority, p.coeff_worddistance,
            p.coeff_appurl, p.coeff_app_dc_title, p.coeff_app_dc_creator, p.coeff_app_dc_subject,
            p.coeff_app_dc_description, p.coeff_appemph, p.coeff_catindexof, p.coeff_cathasimage,
            p.coeff_cathasaudio, p.coeff_cathasvideo, p.coeff_cathasapp, p.coeff_urlcompintoplist,
            p.coeff_descrcompintoplist, p.coeff_prefer, p.coeff_termfrequency, p.coeff_language, p.coeff_citation};
    }

    private static byte[] flatten(final byte[][] hashes) {
        final byte[] b = new byte[12 * hashes.length];
        for (int i = 0; i < hashes.length; i++) System.arraycopy(hashes[i], 0, b, 12 * i, 12);
        return b;
    }

    /** the 12-byte hashes of every query back to back (a null query: none) */
    private static byte[] flatten3(final byte[][][] hashes) {
        int n = 0;
        for (final byte[][] q : hashes) n += q == null ? 0 : q.length;
        final byte[] b = new byte[12 * n];
        int k = 0;
        for (final byte[][] q : hashes) {
            if (q == null) continue;
            for (final byte[] h : q) System.arraycopy(h, 0, b, 12 * k++, 12);
        }
        return b;
    }

    private static byte[] flattenN(final byte[][] hashes, final int w) {
        if (hashes == null) return null;
        final byte[] b = new byte[w * hashes.length];
        for (int i = 0; i < hashes.length; i++) System.arraycopy(hashes[i], 0, b, w * i, w);
        return b;
    }

    private static void check(final int rc) {
        if (rc != 0) throw new IllegalStateException("libyrwi error " + rc);
    }

    private static native long open(int device);
    private static native void close(long ctx);
    private static native int putList(long ctx, byte[] term, byte[] rows, int n, int sorted);
    private static native long[] addPostings(long ctx, byte[] terms, byte[] rows, int n, int policy);
    private static native long[] removePostings(long ctx, byte[] terms, int nterms, byte[] urls, int nurls);
    private static native long[] removeHosts(long ctx, byte[] terms, int nterms, byte[] hosts6, int nhosts);
    private static native long[] countHosts(long ctx, byte[] terms, int nterms, byte[] hosts6, int nhosts);
    private static native long[] urlReferences(long ctx, byte[] terms, int nterms, byte[] urls, int nurls, int order,
                                               long cap, byte[] terms12, byte[] rows40);
    // {nout, the 11 statistics, counts[0 .. nout)}; hosts6Out (6 * cap bytes) receives the hosts; null: failed
    private static native long[] hostCensus(long ctx, byte[] terms, int nterms, int order, long minPostings, long cap,
                                            byte[] hosts6Out);
    // the 15 statistics, then with hist != 0 the 65536 histogram entries; null: failed
    private static native long[] retentionCount(long ctx, byte[] terms, int nterms, int minDay, long maxRefs, int hist);
    // the 9 statistics of removePostings, then the 15 of retentionCount; null: failed
    private static native long[] retain(long ctx, byte[] terms, int nterms, int minDay, long maxRefs);
    private static native byte[] joinExclude(long ctx, byte[] incl, int nincl, byte[] excl, int nexcl,
                                             int maxDistance, long nowMillis);
    private static native long[] normalizeScore(long ctx, byte[] rows, int m, int[] profile32, String language,
                                                long nowMillis);
    private static native byte[] termSearch(long ctx, byte[] incl, int nincl, byte[] excl, int nexcl, byte[] sel,
                                            int nsel, int maxDistance, long nowMillis);
    private static native byte[] termSearchBatch(long ctx, int nq, byte[] incl, int[] nincl, byte[] excl, int[] nexcl,
                                                 byte[] sel, int[] nsel, int[] maxDistance, long[] nowMillis,
                                                 long[] rowOff);
    private static native Object[] hostFacets(long ctx, int nq, byte[] incl, int[] nincl, byte[] excl, int[] nexcl,
                                              byte[] sel, int[] nsel, int[] maxDistance, long[] nowMillis, int order,
                                              int maxHosts, boolean wantUrls, long[] hostOff, long[] nhosts,
                                              long[] nrows, long[] stats);
    private static native long joinExcludeInto(long ctx, byte[] incl, int nincl, byte[] excl, int nexcl,
                                               int maxDistance, long nowMillis, java.nio.ByteBuffer out);
    private static native byte[] query(long ctx, byte[] incl, int nincl, byte[] excl, int nexcl, int maxDistance,
                                       int k, int[] profile32, String language, long nowMillis, long[] stats);
    private static native long[] loadHeaps(long ctx, String[] paths, int byName);
    private static native long[] dumpHeap(long ctx, String path, byte[] terms, int nterms, long nowMs);
    private static native Object[] dhtSelect(long ctx, byte[] start, byte[] limit, int maxContainers, long maxRefs,
                                             int partitionExponent, int flags, long[] stats);
    private static native byte[] queryFiltered(long ctx, byte[] incl, int nincl, byte[] excl, int nexcl,
                                               int maxDistance, int k, int[] profile32, String language,
                                               long nowMillis, byte[] constraint, boolean allOf, int contentdom,
                                               boolean strictDom, String modifierLanguage, byte[] site,
                                               byte[] altSite, byte[] siteExcludes, byte[] urlHashes,
                                               boolean skipDoubleDom, int[] flagCount);
    private static native byte[][] queryRows(long ctx, byte[] incl, int nincl, byte[] excl, int nexcl,
                                             int maxDistance, int k, int[] profile32, String language,
                                             long nowMillis, byte[] constraint, boolean allOf, int contentdom,
                                             boolean strictDom, String modifierLanguage, byte[] site,
                                             byte[] altSite, byte[] siteExcludes, byte[] urlHashes,
                                             boolean skipDoubleDom, int[] flagCount);
    private static native long eventOpen(long ctx, int[] profile32, String language, long nowMillis, int k,
                                         long maxPostings);
    private static native long eventOpenFiltered(long ctx, int[] profile32, String language, long nowMillis, int k,
                                                 long maxPostings, byte[] constraint, boolean allOf, int contentdom,
                                                 boolean strictDom, String modifierLanguage, byte[] site,
                                                 byte[] altSite, byte[] siteExcludes, byte[] urlHashes);
    private static native int[] eventFlagCount(long ctx, long event);
    private static native int[] eventSource(long ctx, long event, byte[] urls, int n);
    private static native long eventOpenOrder(long ctx, int[] profile32, String language, long nowMillis,
                                              long maxHosts);
    private static native int eventAdd(long ctx, long event, byte[] rows, int n, boolean local);
    private static native long eventAddLocal(long ctx, long event, byte[] incl, int nincl, byte[] excl, int nexcl,
                                             byte[] sel, int nsel, int maxDistance, long nowMillis);
    private static native byte[] eventRows(long ctx, long event, byte[] urls, int n);
    private static native byte[] eventResult(long ctx, long event, int maxn);
    private static native long[] eventOrder(long ctx, long event, byte[] rows, int n, boolean local);
    private static native int[] eventAuthority(long ctx, long event, byte[] hosts6, int n);
    private static native byte[] eventPull(long ctx, long event, boolean skipDoubleDom, int maxn);
    private static native void eventClose(long ctx, long event);
    private static native String[] indexAbstracts(long ctx, byte[] words, int nwords, long capacity);
    private static native long[] listSizes(long ctx, byte[] terms, int nterms);
    private static native byte[] getList(long ctx, byte[] term);
    private static native long[] scoreNodes(long ctx, byte[] nodes, int n, int[] profile32, String language,
                                            int maxdomcount);
}
