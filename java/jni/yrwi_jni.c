/* yrwi_jni.c -- JNI glue between net.yacy.kelondro.rwi.GpuRWI and libyrwi.
 * UNVERIFIED (no JDK / jni.h in this image); see INTEGRATION.md.
 * Build on a JDK host:
 *   cc -O2 -shared -fPIC -I$JAVA_HOME/include -I$JAVA_HOME/include/linux -I../../include \
 *      yrwi_jni.c -L../../yacy_search_server_amd -lyrwi -o libyrwi_jni.so */
#include <jni.h>
#include <stdlib.h>
#include <string.h>

#include "yrwi.h"

/* A Java byte[] of at least `need` bytes copied into native memory (no critical
 * region around library calls that synchronise with the GPU: GC stays free);
 * NULL (IllegalArgumentException pending) when the array is shorter, or on OOM. */
static uint8_t* copy_in(JNIEnv* env, jbyteArray a, int64_t need) {
  if (a == NULL || need < 0 || (int64_t)(*env)->GetArrayLength(env, a) < need) {
    jclass ex = (*env)->FindClass(env, "java/lang/IllegalArgumentException");
    if (ex) (*env)->ThrowNew(env, ex, "array shorter than n rows / hosts");
    return NULL;
  }
  uint8_t* b = (uint8_t*)malloc((size_t)(need > 0 ? need : 1));
  if (b && need > 0) (*env)->GetByteArrayRegion(env, a, 0, (jsize)need, (jbyte*)b);
  return b;
}

static void to_profile(JNIEnv* env, jintArray a, yrwi_profile* p) {
  if (a == NULL) { yrwi_profile_default(p); return; }
  (*env)->GetIntArrayRegion(env, a, 0, 32, (jint*)p);
}

JNIEXPORT jlong JNICALL Java_net_yacy_kelondro_rwi_GpuRWI_open(JNIEnv* env, jclass c, jint dev) {
  yrwi_ctx* ctx = NULL;
  return yrwi_open(dev, &ctx) == 0 ? (jlong)(intptr_t)ctx : 0;
}

JNIEXPORT void JNICALL Java_net_yacy_kelondro_rwi_GpuRWI_close(JNIEnv* env, jclass c, jlong ctx) {
  yrwi_close((yrwi_ctx*)(intptr_t)ctx);
}

JNIEXPORT jint JNICALL Java_net_yacy_kelondro_rwi_GpuRWI_putList(JNIEnv* env, jclass c, jlong ctx, jbyteArray term,
                                                                jbyteArray rows, jint n, jint sorted) {
  jbyte t[12];
  (*env)->GetByteArrayRegion(env, term, 0, 12, t);
  uint8_t* p = copy_in(env, rows, (int64_t)n * 40);
  if (!p) return YRWI_E_ARG;
  int rc = yrwi_put_list((yrwi_ctx*)(intptr_t)ctx, (const uint8_t*)t, p, n, sorted);
  free(p);
  return rc;
}

/* ---- index updates on the device (yrwi_add_postings / yrwi_remove_postings / yrwi_remove_hosts /
 *      yrwi_count_hosts) ---- */
/* yrwi_update_stats as long[9]: terms, new_terms, emptied_terms, added, replaced, dropped, removed,
 * launches, syncs; NULL when rc != 0 */
static jlongArray update_stats(JNIEnv* env, int rc, const yrwi_update_stats* st) {
  if (rc != 0) return NULL;
  const jlong v[9] = {st->terms, st->new_terms, st->emptied_terms, st->added, st->replaced,
                      st->dropped, st->removed, st->launches, st->syncs};
  jlongArray res = (*env)->NewLongArray(env, 9);
  if (res) (*env)->SetLongArrayRegion(env, res, 0, 9, v);
  return res;
}

JNIEXPORT jlongArray JNICALL Java_net_yacy_kelondro_rwi_GpuRWI_addPostings(JNIEnv* env, jclass c, jlong ctx,
                                                                          jbyteArray terms, jbyteArray rows, jint n,
                                                                          jint policy) {
  /* both arrays are copied out of the Java heap: the call synchronises with the GPU */
  uint8_t* t = copy_in(env, terms, (int64_t)n * 12);
  if (!t) return NULL;
  uint8_t* r = copy_in(env, rows, (int64_t)n * 40);
  if (!r) {
    free(t);
    return NULL;
  }
  yrwi_update_stats st;
  int rc = yrwi_add_postings((yrwi_ctx*)(intptr_t)ctx, t, r, n, policy, &st);
  free(t);
  free(r);
  return update_stats(env, rc, &st);
}

JNIEXPORT jlongArray JNICALL Java_net_yacy_kelondro_rwi_GpuRWI_removePostings(JNIEnv* env, jclass c, jlong ctx,
                                                                             jbyteArray terms, jint nterms,
                                                                             jbyteArray urls, jint nurls) {
  uint8_t* t = copy_in(env, terms, (int64_t)nterms * 12);
  if (!t) return NULL;
  uint8_t* u = copy_in(env, urls, (int64_t)nurls * 12);
  if (!u) {
    free(t);
    return NULL;
  }
  yrwi_update_stats st;
  int rc = yrwi_remove_postings((yrwi_ctx*)(intptr_t)ctx, t, nterms, u, nurls, &st);
  free(t);
  free(u);
  return update_stats(env, rc, &st);
}

/* yrwi_remove_hosts: hosts = nhosts * 6 bytes (url-hash characters 6..11); the statistics of removePostings */
JNIEXPORT jlongArray JNICALL Java_net_yacy_kelondro_rwi_GpuRWI_removeHosts(JNIEnv* env, jclass c, jlong ctx,
                                                                          jbyteArray terms, jint nterms,
                                                                          jbyteArray hosts, jint nhosts) {
  uint8_t* t = copy_in(env, terms, (int64_t)nterms * 12);
  if (!t) return NULL;
  uint8_t* h = copy_in(env, hosts, (int64_t)nhosts * 6);
  if (!h) {
    free(t);
    return NULL;
  }
  yrwi_update_stats st;
  int rc = yrwi_remove_hosts((yrwi_ctx*)(intptr_t)ctx, t, nterms, h, nhosts, &st);
  free(t);
  free(h);
  return update_stats(env, rc, &st);
}

/* yrwi_count_hosts as long[nhosts + 1]: the postings of every host in the selected lists, then the
 * selected lists that hold at least one of them; NULL when the call failed */
JNIEXPORT jlongArray JNICALL Java_net_yacy_kelondro_rwi_GpuRWI_countHosts(JNIEnv* env, jclass c, jlong ctx,
                                                                         jbyteArray terms, jint nterms,
                                                                         jbyteArray hosts, jint nhosts) {
  uint8_t* t = copy_in(env, terms, (int64_t)nterms * 12);
  if (!t) return NULL;
  uint8_t* h = copy_in(env, hosts, (int64_t)nhosts * 6);
  if (!h) {
    free(t);
    return NULL;
  }
  jlong* v = (jlong*)calloc((size_t)nhosts + 1, sizeof(jlong));
  int64_t hit = 0;
  int rc = v ? yrwi_count_hosts((yrwi_ctx*)(intptr_t)ctx, t, nterms, h, nhosts, (int64_t*)v, &hit) : YRWI_E_NOMEM;
  free(t);
  free(h);
  jlongArray res = NULL;
  if (rc == 0) {
    v[nhosts] = hit;
    res = (*env)->NewLongArray(env, nhosts + 1);
    if (res) (*env)->SetLongArrayRegion(env, res, 0, nhosts + 1, v);
  }
  free(v);
  return res;
}

/* yrwi_url_references as long[16 + nurls]: yrwi_ref_stats (lists, postings, urls, urls_found, refs, lists_hit,
 * lists_covered, path, direct, launches, syncs, bytes_h2d, bytes_d2h, t_find_ns, t_total_ns), the call's return
 * code (0, or YRWI_E_ARG when refs > cap and nothing was fetched), then the references of every url.  With
 * cap > 0 the references' terms go into terms12 (at least 12 * cap bytes) and their rows into rows40 (at least
 * 40 * cap bytes), in `order`; cap == 0 only counts (the arrays may be null).  NULL when the call failed otherwise */
JNIEXPORT jlongArray JNICALL Java_net_yacy_kelondro_rwi_GpuRWI_urlReferences(JNIEnv* env, jclass c, jlong ctx,
                                                                            jbyteArray terms, jint nterms,
                                                                            jbyteArray urls, jint nurls, jint order,
                                                                            jlong cap, jbyteArray terms12,
                                                                            jbyteArray rows40) {
  if (cap < 0 || (cap > 0 && (!terms12 || !rows40 || (jlong)(*env)->GetArrayLength(env, terms12) < 12 * cap ||
                              (jlong)(*env)->GetArrayLength(env, rows40) < 40 * cap)))
    return NULL;
  uint8_t* t = copy_in(env, terms, (int64_t)nterms * 12);
  if (!t) return NULL;
  uint8_t* u = copy_in(env, urls, (int64_t)nurls * 12);
  if (!u) {
    free(t);
    return NULL;
  }
  uint8_t* to = (uint8_t*)malloc((size_t)cap * 12 + 1);
  uint8_t* ro = (uint8_t*)malloc((size_t)cap * 40 + 1);
  jlong* v = (jlong*)calloc((size_t)nurls + 16, sizeof(jlong));
  yrwi_ref_stats st;
  int rc = to && ro && v ? yrwi_url_references((yrwi_ctx*)(intptr_t)ctx, t, nterms, u, nurls, order, (int64_t*)(v + 16),
                                               cap ? to : NULL, cap ? ro : NULL, cap, &st)
                         : YRWI_E_NOMEM;
  free(t);
  free(u);
  jlongArray res = NULL;
  if (rc == 0 || (rc == YRWI_E_ARG && cap > 0 && st.refs > cap)) {
    const jlong s[16] = {st.lists, st.postings, st.urls,      st.urls_found, st.refs,      st.lists_hit,
                         st.lists_covered, st.path, st.direct, st.launches,  st.syncs,     st.bytes_h2d,
                         st.bytes_d2h,     st.t_find_ns,       st.t_total_ns, rc};
    memcpy(v, s, sizeof(s));
    if (rc == 0 && cap > 0 && st.refs > 0) {
      (*env)->SetByteArrayRegion(env, terms12, 0, (jsize)(12 * st.refs), (const jbyte*)to);
      (*env)->SetByteArrayRegion(env, rows40, 0, (jsize)(40 * st.refs), (const jbyte*)ro);
    }
    res = (*env)->NewLongArray(env, (jsize)(16 + nurls));
    if (res) (*env)->SetLongArrayRegion(env, res, 0, (jsize)(16 + nurls), v);
  }
  free(to);
  free(ro);
  free(v);
  return res;
}

/* yrwi_host_census as long[12 + nout]: nout, then yrwi_census_stats (lists, postings, hosts, hosts_passing,
 * table_slots, passes, lds_bypass, launches, syncs, t_count_ns, t_total_ns), then the nout counts; the hosts
 * (6 bytes each) go into hosts6 (at least 6 * cap bytes); NULL when the call failed */
JNIEXPORT jlongArray JNICALL Java_net_yacy_kelondro_rwi_GpuRWI_hostCensus(JNIEnv* env, jclass c, jlong ctx,
                                                                         jbyteArray terms, jint nterms, jint order,
                                                                         jlong min_postings, jlong cap,
                                                                         jbyteArray hosts6) {
  if (cap < 0 || (cap > 0 && (!hosts6 || (jlong)(*env)->GetArrayLength(env, hosts6) < 6 * cap))) return NULL;
  uint8_t* t = copy_in(env, terms, (int64_t)nterms * 12);
  if (!t) return NULL;
  uint8_t* h = (uint8_t*)malloc((size_t)cap * 6 + 1);
  jlong* v = (jlong*)calloc((size_t)cap + 12, sizeof(jlong));
  yrwi_census_stats st;
  int64_t n = 0;
  int rc = h && v ? yrwi_host_census((yrwi_ctx*)(intptr_t)ctx, t, nterms, order, min_postings, cap ? h : NULL,
                                     cap ? (int64_t*)(v + 12) : NULL, cap, &n, &st)
                  : YRWI_E_NOMEM;
  free(t);
  jlongArray res = NULL;
  if (rc == 0) {
    const jlong s[12] = {n, st.lists, st.postings, st.hosts, st.hosts_passing, st.table_slots, st.passes,
                         st.lds_bypass, st.launches, st.syncs, st.t_count_ns, st.t_total_ns};
    memcpy(v, s, sizeof(s));
    if (n > 0) (*env)->SetByteArrayRegion(env, hosts6, 0, (jsize)(6 * n), (const jbyte*)h);
    res = (*env)->NewLongArray(env, (jsize)(12 + n));
    if (res) (*env)->SetLongArrayRegion(env, res, 0, (jsize)(12 + n), v);
  }
  free(h);
  free(v);
  return res;
}

/* yrwi_retention_stats as 15 longs at v: lists, postings, removed_age, removed_cap, lists_age, lists_cap,
 * emptied_terms, day_min, day_max, launches, syncs, t_mark_ns, t_select_ns, t_total_ns, hist_bypass */
static void retention_stats(jlong* v, const yrwi_retention_stats* st) {
  const jlong s[15] = {st->lists,     st->postings,      st->removed_age, st->removed_cap, st->lists_age,
                       st->lists_cap, st->emptied_terms, st->day_min,     st->day_max,     st->launches,
                       st->syncs,     st->t_mark_ns,     st->t_select_ns, st->t_total_ns,  st->hist_bypass};
  memcpy(v, s, sizeof(s));
}

/* yrwi_retention_count as long[15], or with hist != 0 as long[15 + 65536]: the statistics, then the histogram
 * of the selected rows' lastModified days; NULL when the call failed */
JNIEXPORT jlongArray JNICALL Java_net_yacy_kelondro_rwi_GpuRWI_retentionCount(JNIEnv* env, jclass c, jlong ctx,
                                                                             jbyteArray terms, jint nterms,
                                                                             jint min_day, jlong max_refs, jint hist) {
  uint8_t* t = copy_in(env, terms, (int64_t)nterms * 12);
  if (!t) return NULL;
  const jsize n = 15 + (hist ? 65536 : 0);
  jlong* v = (jlong*)calloc((size_t)n, sizeof(jlong));
  yrwi_retention_stats st;
  int rc = v ? yrwi_retention_count((yrwi_ctx*)(intptr_t)ctx, t, nterms, min_day, max_refs,
                                    hist ? (int64_t*)(v + 15) : NULL, &st)
             : YRWI_E_NOMEM;
  free(t);
  jlongArray res = NULL;
  if (rc == 0) {
    retention_stats(v, &st);
    res = (*env)->NewLongArray(env, n);
    if (res) (*env)->SetLongArrayRegion(env, res, 0, n, v);
  }
  free(v);
  return res;
}

/* yrwi_retain as long[9 + 15]: the statistics of removePostings, then yrwi_retention_stats; NULL when the call
 * failed */
JNIEXPORT jlongArray JNICALL Java_net_yacy_kelondro_rwi_GpuRWI_retain(JNIEnv* env, jclass c, jlong ctx,
                                                                     jbyteArray terms, jint nterms, jint min_day,
                                                                     jlong max_refs) {
  uint8_t* t = copy_in(env, terms, (int64_t)nterms * 12);
  if (!t) return NULL;
  yrwi_update_stats st;
  yrwi_retention_stats rst;
  int rc = yrwi_retain((yrwi_ctx*)(intptr_t)ctx, t, nterms, min_day, max_refs, &st, &rst);
  free(t);
  if (rc != 0) return NULL;
  jlong v[24] = {st.terms, st.new_terms, st.emptied_terms, st.added, st.replaced, st.dropped, st.removed,
                 st.launches, st.syncs};
  retention_stats(v + 9, &rst);
  jlongArray res = (*env)->NewLongArray(env, 24);
  if (res) (*env)->SetLongArrayRegion(env, res, 0, 24, v);
  return res;
}

JNIEXPORT jbyteArray JNICALL Java_net_yacy_kelondro_rwi_GpuRWI_joinExclude(JNIEnv* env, jclass c, jlong ctx,
                                                                          jbyteArray incl, jint nincl, jbyteArray excl,
                                                                          jint nexcl, jint maxd, jlong now) {
  yrwi_ctx* x = (yrwi_ctx*)(intptr_t)ctx;
  jbyte* ib = (*env)->GetByteArrayElements(env, incl, NULL);
  jbyte* eb = (*env)->GetByteArrayElements(env, excl, NULL);
  int64_t cap = 0, n;
  for (int i = 0; i < nincl; i++) {
    if (yrwi_list_size(x, (const uint8_t*)ib + 12 * i, &n) == 0 && n > cap) cap = n;
  }
  uint8_t* out = (uint8_t*)malloc((size_t)(cap > 0 ? cap : 1) * 40);
  int64_t m = 0;
  int rc = yrwi_join_exclude(x, (const uint8_t*)ib, nincl, (const uint8_t*)eb, nexcl, maxd, now, out, cap, &m);
  (*env)->ReleaseByteArrayElements(env, incl, ib, JNI_ABORT);
  (*env)->ReleaseByteArrayElements(env, excl, eb, JNI_ABORT);
  jbyteArray res = NULL;
  if (rc == 0) {
    res = (*env)->NewByteArray(env, (jsize)(m * 40));
    (*env)->SetByteArrayRegion(env, res, 0, (jsize)(m * 40), (const jbyte*)out);
  }
  free(out);
  return res;  /* null on error (caller: yrwi_last_error) */
}

/* TermSearch(..., urlselection, ...).joined(): every list restricted to the url
 * selection (n * 12 bytes) before the conjunction (yrwi_term_search) */
JNIEXPORT jbyteArray JNICALL Java_net_yacy_kelondro_rwi_GpuRWI_termSearch(JNIEnv* env, jclass c, jlong ctx,
                                                                         jbyteArray incl, jint nincl, jbyteArray excl,
                                                                         jint nexcl, jbyteArray sel, jint nsel,
                                                                         jint maxd, jlong now) {
  yrwi_ctx* x = (yrwi_ctx*)(intptr_t)ctx;
  jbyte* ib = (*env)->GetByteArrayElements(env, incl, NULL);
  jbyte* eb = (*env)->GetByteArrayElements(env, excl, NULL);
  jbyte* sb = sel ? (*env)->GetByteArrayElements(env, sel, NULL) : NULL;
  int64_t cap = 0, n;
  for (int i = 0; i < nincl; i++) {
    if (yrwi_list_size(x, (const uint8_t*)ib + 12 * i, &n) == 0 && n > cap) cap = n;
  }
  uint8_t* out = (uint8_t*)malloc((size_t)(cap > 0 ? cap : 1) * 40);
  yrwi_query_desc q;
  memset(&q, 0, sizeof(q));
  q.incl = (const uint8_t*)ib; q.nincl = nincl;
  q.excl = (const uint8_t*)eb; q.nexcl = nexcl;
  q.max_distance = maxd; q.k = 1; q.now_ms = now;
  q.urlselection = (const uint8_t*)sb; q.nurlselection = sb ? nsel : 0;
  int64_t m = 0;
  int rc = out ? yrwi_term_search(x, &q, out, cap, &m) : YRWI_E_NOMEM;
  (*env)->ReleaseByteArrayElements(env, incl, ib, JNI_ABORT);
  (*env)->ReleaseByteArrayElements(env, excl, eb, JNI_ABORT);
  if (sb) (*env)->ReleaseByteArrayElements(env, sel, sb, JNI_ABORT);
  jbyteArray res = NULL;
  if (rc == 0) {
    res = (*env)->NewByteArray(env, (jsize)(m * 40));
    (*env)->SetByteArrayRegion(env, res, 0, (jsize)(m * 40), (const jbyte*)out);
  }
  free(out);
  return res;
}

/* TermSearch.joined() of nq queries in one pass (yrwi_term_search_batch).  The term and url
 * hashes of all queries lie back to back in incl / excl / sel (12 bytes each), nincl[i] /
 * nexcl[i] / nsel[i] of them belong to query i (sel and nsel may be NULL: no selection).
 * Returns the packed rows of all queries (rowOff[nq] * 40 bytes) and fills rowOff (nq + 1):
 * query i owns rows rowOff[i] .. rowOff[i + 1].  The buffer is sized by the sum of each
 * query's smallest include list, so no counting call comes first.  NULL on error. */
JNIEXPORT jbyteArray JNICALL Java_net_yacy_kelondro_rwi_GpuRWI_termSearchBatch(
    JNIEnv* env, jclass c, jlong ctx, jint nq, jbyteArray incl, jintArray nincl, jbyteArray excl, jintArray nexcl,
    jbyteArray sel, jintArray nsel, jintArray maxd, jlongArray now, jlongArray rowOff) {
  yrwi_ctx* x = (yrwi_ctx*)(intptr_t)ctx;
  if (nq < 0 || !incl || !nincl || !excl || !nexcl || !maxd || !now || !rowOff || (sel && !nsel) ||
      (*env)->GetArrayLength(env, nincl) < nq || (*env)->GetArrayLength(env, nexcl) < nq ||
      (*env)->GetArrayLength(env, maxd) < nq || (*env)->GetArrayLength(env, now) < nq ||
      (*env)->GetArrayLength(env, rowOff) < nq + 1 || (sel && (*env)->GetArrayLength(env, nsel) < nq))
    return NULL;
  jint* ni = (*env)->GetIntArrayElements(env, nincl, NULL);
  jint* ne = (*env)->GetIntArrayElements(env, nexcl, NULL);
  jint* ns = sel ? (*env)->GetIntArrayElements(env, nsel, NULL) : NULL;
  jint* md = (*env)->GetIntArrayElements(env, maxd, NULL);
  jlong* nw = (*env)->GetLongArrayElements(env, now, NULL);
  int64_t ti = 0, te = 0, ts = 0;
  int ok = 1;
  for (jint i = 0; i < nq; i++) {
    if (ni[i] < 0 || ne[i] < 0 || (ns && ns[i] < 0)) ok = 0;
    ti += ni[i];
    te += ne[i];
    ts += ns ? ns[i] : 0;
  }
  uint8_t* ib = ok ? copy_in(env, incl, ti * 12) : NULL;
  uint8_t* eb = ib ? copy_in(env, excl, te * 12) : NULL;
  uint8_t* sb = eb && sel ? copy_in(env, sel, ts * 12) : NULL;
  yrwi_query_desc* q = (yrwi_query_desc*)calloc((size_t)nq + 1, sizeof(yrwi_query_desc));
  int64_t* off = (int64_t*)calloc((size_t)nq + 1, sizeof(int64_t));
  uint8_t* out = NULL;
  int rc = ib && eb && (!sel || sb) && q && off ? 0 : YRWI_E_NOMEM;
  int64_t cap = 0;
  if (rc == 0) {
    int64_t oi = 0, oe = 0, os = 0;
    for (jint i = 0; i < nq; i++) {
      q[i].incl = ib + 12 * oi; q[i].nincl = ni[i];
      q[i].excl = eb + 12 * oe; q[i].nexcl = ne[i];
      q[i].max_distance = md[i]; q[i].k = 1; q[i].now_ms = nw[i];
      if (ns && ns[i] > 0) { q[i].urlselection = sb + 12 * os; q[i].nurlselection = ns[i]; }
      int64_t least = 0, n;  /* a conjunction is no longer than its shortest include list */
      for (int t = 0; t < ni[i]; t++) {
        n = 0;
        yrwi_list_size(x, q[i].incl + 12 * t, &n);
        if (t == 0 || n < least) least = n;
      }
      cap += least;
      oi += ni[i]; oe += ne[i]; os += ns ? ns[i] : 0;
    }
    out = (uint8_t*)malloc((size_t)(cap > 0 ? cap : 1) * 40);
    rc = out ? yrwi_term_search_batch(x, q, nq, out, cap, off, NULL) : YRWI_E_NOMEM;
  }
  (*env)->ReleaseIntArrayElements(env, nincl, ni, JNI_ABORT);
  (*env)->ReleaseIntArrayElements(env, nexcl, ne, JNI_ABORT);
  if (ns) (*env)->ReleaseIntArrayElements(env, nsel, ns, JNI_ABORT);
  (*env)->ReleaseIntArrayElements(env, maxd, md, JNI_ABORT);
  (*env)->ReleaseLongArrayElements(env, now, nw, JNI_ABORT);
  jbyteArray res = NULL;
  if (rc == 0 && off[nq] * 40 <= 0x7FFFFFFF) {
    res = (*env)->NewByteArray(env, (jsize)(off[nq] * 40));
    if (res) {
      (*env)->SetByteArrayRegion(env, res, 0, (jsize)(off[nq] * 40), (const jbyte*)out);
      (*env)->SetLongArrayRegion(env, rowOff, 0, nq + 1, (const jlong*)off);
    }
  }
  free(ib);
  free(eb);
  free(sb);
  free(q);
  free(off);
  free(out);
  return res;
}

/* The hosts of the joined container of nq queries and their postings (yrwi_host_facets_batch).
 * The queries are given as for termSearchBatch.  order: YRWI_FACETS_BY_*; maxHosts: the most
 * hosts per query (0: all); wantUrls: each host's smallest url hash as well.  Sized by a counting
 * call.  Returns Object[3] {byte[] hosts (n * 6), long[] counts (n), byte[] urls (n * 12) or
 * null}, n = hostOff[nq], and fills hostOff (nq + 1), nhosts and nrows (nq each, or null) and
 * stats (long[11] or null: the fields of yrwi_facet_stats in their order); NULL on error. */
JNIEXPORT jobjectArray JNICALL Java_net_yacy_kelondro_rwi_GpuRWI_hostFacets(
    JNIEnv* env, jclass c, jlong ctx, jint nq, jbyteArray incl, jintArray nincl, jbyteArray excl, jintArray nexcl,
    jbyteArray sel, jintArray nsel, jintArray maxd, jlongArray now, jint order, jint maxHosts, jboolean wantUrls,
    jlongArray hostOff, jlongArray nhosts, jlongArray nrows, jlongArray stats) {
  yrwi_ctx* x = (yrwi_ctx*)(intptr_t)ctx;
  if (nq < 0 || !incl || !nincl || !excl || !nexcl || !maxd || !now || !hostOff || (sel && !nsel) ||
      (*env)->GetArrayLength(env, nincl) < nq || (*env)->GetArrayLength(env, nexcl) < nq ||
      (*env)->GetArrayLength(env, maxd) < nq || (*env)->GetArrayLength(env, now) < nq ||
      (*env)->GetArrayLength(env, hostOff) < nq + 1 || (sel && (*env)->GetArrayLength(env, nsel) < nq) ||
      (nhosts && (*env)->GetArrayLength(env, nhosts) < nq) || (nrows && (*env)->GetArrayLength(env, nrows) < nq))
    return NULL;
  jint* ni = (*env)->GetIntArrayElements(env, nincl, NULL);
  jint* ne = (*env)->GetIntArrayElements(env, nexcl, NULL);
  jint* ns = sel ? (*env)->GetIntArrayElements(env, nsel, NULL) : NULL;
  jint* md = (*env)->GetIntArrayElements(env, maxd, NULL);
  jlong* nw = (*env)->GetLongArrayElements(env, now, NULL);
  int64_t ti = 0, te = 0, ts = 0;
  int ok = 1;
  for (jint i = 0; i < nq; i++) {
    if (ni[i] < 0 || ne[i] < 0 || (ns && ns[i] < 0)) ok = 0;
    ti += ni[i];
    te += ne[i];
    ts += ns ? ns[i] : 0;
  }
  uint8_t* ib = ok ? copy_in(env, incl, ti * 12) : NULL;
  uint8_t* eb = ib ? copy_in(env, excl, te * 12) : NULL;
  uint8_t* sb = eb && sel ? copy_in(env, sel, ts * 12) : NULL;
  yrwi_query_desc* q = (yrwi_query_desc*)calloc((size_t)nq + 1, sizeof(yrwi_query_desc));
  int64_t* off = (int64_t*)calloc(3 * (size_t)nq + 3, sizeof(int64_t)); /* hostOff, nhosts, nrows */
  int64_t *nh = off ? off + nq + 1 : NULL, *nr = off ? off + 2 * (size_t)nq + 2 : NULL;
  uint8_t *h6 = NULL, *u12 = NULL;
  int64_t* cnt = NULL;
  yrwi_facet_stats st;
  memset(&st, 0, sizeof(st));
  int rc = ib && eb && (!sel || sb) && q && off ? 0 : YRWI_E_NOMEM;
  if (rc == 0) {
    int64_t oi = 0, oe = 0, os = 0;
    for (jint i = 0; i < nq; i++) {
      q[i].incl = ib + 12 * oi; q[i].nincl = ni[i];
      q[i].excl = eb + 12 * oe; q[i].nexcl = ne[i];
      q[i].max_distance = md[i]; q[i].k = 1; q[i].now_ms = nw[i];
      if (ns && ns[i] > 0) { q[i].urlselection = sb + 12 * os; q[i].nurlselection = ns[i]; }
      oi += ni[i]; oe += ne[i]; os += ns ? ns[i] : 0;
    }
    rc = yrwi_host_facets_batch(x, q, nq, order, maxHosts, NULL, NULL, NULL, 0, off, NULL, NULL, NULL); /* counts only */
  }
  (*env)->ReleaseIntArrayElements(env, nincl, ni, JNI_ABORT);
  (*env)->ReleaseIntArrayElements(env, nexcl, ne, JNI_ABORT);
  if (ns) (*env)->ReleaseIntArrayElements(env, nsel, ns, JNI_ABORT);
  (*env)->ReleaseIntArrayElements(env, maxd, md, JNI_ABORT);
  (*env)->ReleaseLongArrayElements(env, now, nw, JNI_ABORT);
  const int64_t n = rc == 0 ? off[nq] : 0;
  if (rc == 0 && n * 12 > 2147483647LL) rc = YRWI_E_LIMIT; /* a Java array holds at most 2^31 - 1 elements */
  if (rc == 0) {
    h6 = (uint8_t*)malloc((size_t)(n > 0 ? n * 6 : 1));
    cnt = (int64_t*)malloc((size_t)(n > 0 ? n : 1) * sizeof(int64_t));
    u12 = wantUrls ? (uint8_t*)malloc((size_t)(n > 0 ? n * 12 : 1)) : NULL;
    rc = h6 && cnt && (!wantUrls || u12)
             ? yrwi_host_facets_batch(x, q, nq, order, maxHosts, h6, cnt, u12, n, off, nh, nr, &st)
             : YRWI_E_NOMEM;
  }
  jobjectArray res = NULL;
  if (rc == 0) {
    jclass oc = (*env)->FindClass(env, "java/lang/Object");
    jbyteArray jh = (*env)->NewByteArray(env, (jsize)(n * 6));
    jlongArray jc = (*env)->NewLongArray(env, (jsize)n);
    jbyteArray ju = wantUrls ? (*env)->NewByteArray(env, (jsize)(n * 12)) : NULL;
    if (oc && jh && jc && (!wantUrls || ju)) res = (*env)->NewObjectArray(env, 3, oc, NULL);
    if (res) {
      (*env)->SetByteArrayRegion(env, jh, 0, (jsize)(n * 6), (const jbyte*)h6);
      (*env)->SetLongArrayRegion(env, jc, 0, (jsize)n, (const jlong*)cnt);
      if (ju) (*env)->SetByteArrayRegion(env, ju, 0, (jsize)(n * 12), (const jbyte*)u12);
      (*env)->SetObjectArrayElement(env, res, 0, jh);
      (*env)->SetObjectArrayElement(env, res, 1, jc);
      (*env)->SetObjectArrayElement(env, res, 2, ju);
      (*env)->SetLongArrayRegion(env, hostOff, 0, nq + 1, (const jlong*)off);
      if (nhosts) (*env)->SetLongArrayRegion(env, nhosts, 0, nq, (const jlong*)nh);
      if (nrows) (*env)->SetLongArrayRegion(env, nrows, 0, nq, (const jlong*)nr);
      if (stats && (*env)->GetArrayLength(env, stats) >= 11) {
        const jlong v[11] = {st.rows_joined, st.rows_kept, st.hosts, st.hosts_out, st.bytes_h2d, st.bytes_d2h,
                             st.launches_tail, st.syncs, st.device_allocs, st.t_group_ns, st.t_total_ns};
        (*env)->SetLongArrayRegion(env, stats, 0, 11, v);
      }
    }
  }
  free(ib);
  free(eb);
  free(sb);
  free(q);
  free(off);
  free(h6);
  free(cnt);
  free(u12);
  return res;
}

/* joinExclude into a direct ByteBuffer the caller owns and reuses (no JNI array copy
 * of the joined container): returns m (rows written, 40 bytes each) or the (negative)
 * error code -- YRWI_E_ARG when the container holds more rows than capacity / 40. */
JNIEXPORT jlong JNICALL Java_net_yacy_kelondro_rwi_GpuRWI_joinExcludeInto(JNIEnv* env, jclass c, jlong ctx,
                                                                         jbyteArray incl, jint nincl,
                                                                         jbyteArray excl, jint nexcl, jint maxd,
                                                                         jlong now, jobject out) {
  uint8_t* dst = (uint8_t*)(*env)->GetDirectBufferAddress(env, out);
  const jlong capb = (*env)->GetDirectBufferCapacity(env, out);
  if (dst == NULL || capb < 0) return YRWI_E_ARG;
  jbyte* ib = (*env)->GetByteArrayElements(env, incl, NULL);
  jbyte* eb = (*env)->GetByteArrayElements(env, excl, NULL);
  int64_t m = 0;
  int rc = yrwi_join_exclude((yrwi_ctx*)(intptr_t)ctx, (const uint8_t*)ib, nincl, (const uint8_t*)eb, nexcl, maxd, now,
                             dst, capb / 40, &m);
  (*env)->ReleaseByteArrayElements(env, incl, ib, JNI_ABORT);
  (*env)->ReleaseByteArrayElements(env, excl, eb, JNI_ABORT);
  return rc == 0 ? (jlong)m : (jlong)rc;
}

/* yrwi_stats -> long[]: postings_in, joined, bytes_alg, bytes_join, t_join_ns, t_norm_ns,
 * t_score_ns, t_total_ns, n_join_launches, n_enum_steps, n_test_steps, n_realloc,
 * bytes_probe, t_probe_ns, bytes_compact, t_compact_ns, t_kernels_ns (17 values) */
#define YRWI_JNI_NSTATS 17
static void stats_out(JNIEnv* env, jlongArray a, const yrwi_stats* st) {
  if (a == NULL) return;
  const jlong v[YRWI_JNI_NSTATS] = {st->postings_in, st->joined, st->bytes_alg, st->bytes_join, st->t_join_ns,
                                    st->t_norm_ns, st->t_score_ns, st->t_total_ns, st->n_join_launches,
                                    st->n_enum_steps, st->n_test_steps, st->n_realloc, st->bytes_probe,
                                    st->t_probe_ns, st->bytes_compact, st->t_compact_ns, st->t_kernels_ns};
  jsize n = (*env)->GetArrayLength(env, a);
  (*env)->SetLongArrayRegion(env, a, 0, n < YRWI_JNI_NSTATS ? n : YRWI_JNI_NSTATS, v);
}

JNIEXPORT jlongArray JNICALL Java_net_yacy_kelondro_rwi_GpuRWI_normalizeScore(JNIEnv* env, jclass c, jlong ctx,
                                                                             jbyteArray rows, jint m, jintArray prof,
                                                                             jstring lang, jlong now) {
  yrwi_profile p;
  to_profile(env, prof, &p);
  const char* l = (*env)->GetStringUTFChars(env, lang, NULL);
  uint8_t* r = copy_in(env, rows, (int64_t)m * 40);
  if (!r) { (*env)->ReleaseStringUTFChars(env, lang, l); return NULL; }
  jlong* sc = (jlong*)malloc(sizeof(jlong) * (size_t)(m > 0 ? m : 1));
  int rc = sc ? yrwi_normalize_score((yrwi_ctx*)(intptr_t)ctx, r, m, &p, l, now, (int64_t*)sc) : YRWI_E_NOMEM;
  free(r);
  (*env)->ReleaseStringUTFChars(env, lang, l);
  jlongArray res = NULL;
  if (rc == 0) {
    res = (*env)->NewLongArray(env, m);
    (*env)->SetLongArrayRegion(env, res, 0, m, sc);
  }
  free(sc);
  return res;
}

JNIEXPORT jbyteArray JNICALL Java_net_yacy_kelondro_rwi_GpuRWI_query(JNIEnv* env, jclass c, jlong ctx,
                                                                    jbyteArray incl, jint nincl, jbyteArray excl,
                                                                    jint nexcl, jint maxd, jint k, jintArray prof,
                                                                    jstring lang, jlong now, jlongArray stats) {
  yrwi_profile p;
  to_profile(env, prof, &p);
  yrwi_query_desc q;
  memset(&q, 0, sizeof(q));
  jbyte* ib = (*env)->GetByteArrayElements(env, incl, NULL);
  jbyte* eb = (*env)->GetByteArrayElements(env, excl, NULL);
  const char* l = (*env)->GetStringUTFChars(env, lang, NULL);
  q.incl = (const uint8_t*)ib; q.nincl = nincl;
  q.excl = (const uint8_t*)eb; q.nexcl = nexcl;
  q.max_distance = maxd; q.k = k; q.profile = &p; q.now_ms = now;
  strncpy(q.language, l, sizeof(q.language) - 1);
  yrwi_hit* hits = (yrwi_hit*)malloc(sizeof(yrwi_hit) * (size_t)(k > 0 ? k : 1));
  int32_t n = 0;
  yrwi_stats st;
  memset(&st, 0, sizeof(st));
  int rc = yrwi_query((yrwi_ctx*)(intptr_t)ctx, &q, hits, &n, stats ? &st : NULL);
  (*env)->ReleaseByteArrayElements(env, incl, ib, JNI_ABORT);
  (*env)->ReleaseByteArrayElements(env, excl, eb, JNI_ABORT);
  (*env)->ReleaseStringUTFChars(env, lang, l);
  jbyteArray res = NULL;
  if (rc == 0) {
    stats_out(env, stats, &st);
    res = (*env)->NewByteArray(env, (jsize)(n * (jint)sizeof(yrwi_hit)));
    (*env)->SetByteArrayRegion(env, res, 0, (jsize)(n * (jint)sizeof(yrwi_hit)), (const jbyte*)hits);
  }
  free(hits);
  return res;
}

/* IndexCell's BLOB files (ReferenceContainerArray): yrwi_load_heaps; returns the
 * stats as long[7] {files, records, free_records, bad_keys, terms, postings, dropped_terms}. */
JNIEXPORT jlongArray JNICALL Java_net_yacy_kelondro_rwi_GpuRWI_loadHeaps(JNIEnv* env, jclass c, jlong ctx,
                                                                        jobjectArray paths, jint byName) {
  const jsize n = (*env)->GetArrayLength(env, paths);
  const char** p = (const char**)calloc((size_t)(n > 0 ? n : 1), sizeof(char*));
  jstring* js = (jstring*)calloc((size_t)(n > 0 ? n : 1), sizeof(jstring));
  for (jsize i = 0; i < n; i++) {
    js[i] = (jstring)(*env)->GetObjectArrayElement(env, paths, i);
    p[i] = (*env)->GetStringUTFChars(env, js[i], NULL);
  }
  yrwi_load_stats st;
  int rc = yrwi_load_heaps((yrwi_ctx*)(intptr_t)ctx, p, n, byName ? YRWI_LOAD_ORDER_BY_NAME : 0, &st);
  for (jsize i = 0; i < n; i++) (*env)->ReleaseStringUTFChars(env, js[i], p[i]);
  free(p);
  free(js);
  if (rc != 0) return NULL;
  jlong v[7] = {st.files, st.records, st.free_records, st.bad_keys, st.terms, st.postings, st.dropped_terms};
  jlongArray res = (*env)->NewLongArray(env, 7);
  (*env)->SetLongArrayRegion(env, res, 0, 7, v);
  return res;
}

/* The IndexCell dump (FlushThread, IndexCell.java:131-166): yrwi_dump_heap; terms: nterms * 12
 * bytes (nterms == 0: every list); returns the stats as long[8] {terms, postings, bytes, windows,
 * launches, syncs, t_pack_ns, t_total_ns}, NULL when the call failed. */
JNIEXPORT jlongArray JNICALL Java_net_yacy_kelondro_rwi_GpuRWI_dumpHeap(JNIEnv* env, jclass c, jlong ctx,
                                                                       jstring path, jbyteArray terms, jint nterms,
                                                                       jlong nowMs) {
  uint8_t* t = copy_in(env, terms, (int64_t)nterms * 12);
  if (!t) return NULL;
  const char* p = (*env)->GetStringUTFChars(env, path, NULL);
  if (!p) {
    free(t);
    return NULL;
  }
  yrwi_dump_stats st;
  int rc = yrwi_dump_heap((yrwi_ctx*)(intptr_t)ctx, p, t, nterms, nowMs, &st);
  (*env)->ReleaseStringUTFChars(env, path, p);
  free(t);
  if (rc != 0) return NULL;
  const jlong v[8] = {st.terms, st.postings, st.bytes, st.windows, st.launches, st.syncs, st.t_pack_ns, st.t_total_ns};
  jlongArray res = (*env)->NewLongArray(env, 8);
  if (res) (*env)->SetLongArrayRegion(env, res, 0, 8, v);
  return res;
}

/* The DHT send path (Dispatcher.selectContainersEnqueueToBuffer): yrwi_dht_select, sized by a dry
 * run (YRWI_DHT_COUNT_ONLY).  start, limit: 12-byte term hashes; flags: YRWI_DHT_*.  Returns
 * Object[3] {byte[] terms (T * 12), long[] partOff (2^e * T + 1), byte[] rows (postings * 40)} and
 * fills stats (long[10] or null) with {terms, postings, skipped_private, removed, wrapped, windows,
 * launches, syncs, t_pack_ns, t_total_ns}; NULL when the call failed. */
JNIEXPORT jobjectArray JNICALL Java_net_yacy_kelondro_rwi_GpuRWI_dhtSelect(JNIEnv* env, jclass c, jlong ctx,
                                                                          jbyteArray start, jbyteArray limit,
                                                                          jint maxContainers, jlong maxRefs,
                                                                          jint exponent, jint flags,
                                                                          jlongArray stats) {
  uint8_t* s = copy_in(env, start, 12);
  if (!s) return NULL;
  uint8_t* l = copy_in(env, limit, 12);
  if (!l) {
    free(s);
    return NULL;
  }
  yrwi_ctx* x = (yrwi_ctx*)(intptr_t)ctx;
  yrwi_dht_stats st;
  memset(&st, 0, sizeof(st));
  jobjectArray res = NULL;
  uint8_t *terms = NULL, *rows = NULL;
  int64_t* off = NULL;
  int rc = yrwi_dht_select(x, s, l, maxContainers, maxRefs, exponent, (flags | YRWI_DHT_COUNT_ONLY) & ~YRWI_DHT_REMOVE,
                           NULL, 0, NULL, NULL, 0, &st);
  const int64_t T = st.terms, n = st.postings;
  const int64_t noff = rc == 0 ? (((int64_t)1 << exponent) * T + 1) : 0;
  /* a Java array holds at most 2^31 - 1 elements */
  if (rc == 0 && (n * 40 > 2147483647LL || noff > 2147483647LL || T * 12 > 2147483647LL)) rc = YRWI_E_LIMIT;
  if (rc == 0 && !(flags & YRWI_DHT_COUNT_ONLY)) {
    terms = (uint8_t*)malloc((size_t)(T > 0 ? T * 12 : 1));
    off = (int64_t*)malloc((size_t)noff * sizeof(int64_t));
    rows = (uint8_t*)malloc((size_t)(n > 0 ? n * 40 : 1));
    if (!terms || !off || !rows) rc = YRWI_E_NOMEM;
    if (rc == 0) rc = yrwi_dht_select(x, s, l, maxContainers, maxRefs, exponent, flags, terms, (int32_t)T, off, rows, n, &st);
    if (rc == 0) {
      jclass oc = (*env)->FindClass(env, "java/lang/Object");
      jbyteArray jt = (*env)->NewByteArray(env, (jsize)(T * 12));
      jlongArray jo = (*env)->NewLongArray(env, (jsize)noff);
      jbyteArray jr = (*env)->NewByteArray(env, (jsize)(n * 40));
      if (oc && jt && jo && jr) res = (*env)->NewObjectArray(env, 3, oc, NULL);
      if (res) {
        (*env)->SetByteArrayRegion(env, jt, 0, (jsize)(T * 12), (const jbyte*)terms);
        (*env)->SetLongArrayRegion(env, jo, 0, (jsize)noff, (const jlong*)off);
        (*env)->SetByteArrayRegion(env, jr, 0, (jsize)(n * 40), (const jbyte*)rows);
        (*env)->SetObjectArrayElement(env, res, 0, jt);
        (*env)->SetObjectArrayElement(env, res, 1, jo);
        (*env)->SetObjectArrayElement(env, res, 2, jr);
      }
    }
  } else if (rc == 0) { /* the dry run alone: empty arrays */
    jclass oc = (*env)->FindClass(env, "java/lang/Object");
    if (oc) res = (*env)->NewObjectArray(env, 3, oc, NULL);
  }
  if (rc == 0 && stats && (*env)->GetArrayLength(env, stats) >= 10) {
    const jlong v[10] = {st.terms,   st.postings, st.skipped_private, st.removed,   st.wrapped,
                         st.windows, st.launches, st.syncs,           st.t_pack_ns, st.t_total_ns};
    (*env)->SetLongArrayRegion(env, stats, 0, 10, v);
  }
  free(terms);
  free(off);
  free(rows);
  free(s);
  free(l);
  return res;
}

/* SearchEvent.addRWIs constraints + pullOneRWI(skipDoubleDom): query with a yrwi_filter.
 * constraint: 4 Bitfield bytes or null; site / altSite: 6-byte host hashes or null;
 * siteExcludes: n*6 bytes; urlHashes: n*12 bytes; flagCount: int[32] out or null. */
/* rows_out != NULL: yrwi_query_rows, *rows_out = the hits' 40-byte rows (n * 40 bytes, hit order) */
static jbyteArray query_filtered(
    JNIEnv* env, jlong ctx, jbyteArray incl, jint nincl, jbyteArray excl, jint nexcl, jint maxd, jint k,
    jintArray prof, jstring lang, jlong now, jbyteArray constraint, jboolean allOf, jint contentdom,
    jboolean strictDom, jstring modLang, jbyteArray site, jbyteArray altSite, jbyteArray siteExcludes,
    jbyteArray urlHashes, jboolean skipDoubleDom, jintArray flagCount, jbyteArray* rows_out) {
  yrwi_profile p;
  to_profile(env, prof, &p);
  yrwi_filter f;
  memset(&f, 0, sizeof(f));
  if (constraint) { (*env)->GetByteArrayRegion(env, constraint, 0, 4, (jbyte*)f.constraint); f.has_constraint = 1; }
  f.all_of_constraint = allOf;
  f.contentdom = contentdom;
  f.strict_contentdom = strictDom;
  if (modLang) {
    const char* ml = (*env)->GetStringUTFChars(env, modLang, NULL);
    strncpy(f.language, ml, sizeof(f.language) - 1);
    (*env)->ReleaseStringUTFChars(env, modLang, ml);
  }
  if (site) { (*env)->GetByteArrayRegion(env, site, 0, 6, (jbyte*)f.sitehash); f.has_sitehash = 1; }
  if (altSite) { (*env)->GetByteArrayRegion(env, altSite, 0, 6, (jbyte*)f.alt_sitehash); f.has_alt_sitehash = 1; }
  jbyte* sx = siteExcludes ? (*env)->GetByteArrayElements(env, siteExcludes, NULL) : NULL;
  jbyte* uh = urlHashes ? (*env)->GetByteArrayElements(env, urlHashes, NULL) : NULL;
  f.siteexcludes = (const uint8_t*)sx;
  f.nsiteexcludes = sx ? (*env)->GetArrayLength(env, siteExcludes) / 6 : 0;
  f.urlhashes = (const uint8_t*)uh;
  f.nurlhashes = uh ? (*env)->GetArrayLength(env, urlHashes) / 12 : 0;
  f.skip_double_dom = skipDoubleDom;
  int32_t fc[32];
  f.flagcount = flagCount ? fc : NULL;
  yrwi_query_desc q;
  memset(&q, 0, sizeof(q));
  jbyte* ib = (*env)->GetByteArrayElements(env, incl, NULL);
  jbyte* eb = (*env)->GetByteArrayElements(env, excl, NULL);
  const char* l = (*env)->GetStringUTFChars(env, lang, NULL);
  q.incl = (const uint8_t*)ib; q.nincl = nincl;
  q.excl = (const uint8_t*)eb; q.nexcl = nexcl;
  q.max_distance = maxd; q.k = k; q.profile = &p; q.now_ms = now; q.filter = &f;
  strncpy(q.language, l, sizeof(q.language) - 1);
  yrwi_hit* hits = (yrwi_hit*)malloc(sizeof(yrwi_hit) * (size_t)(k > 0 ? k : 1));
  uint8_t* rows = rows_out ? (uint8_t*)malloc((size_t)YRWI_ROW_BYTES * (size_t)(k > 0 ? k : 1)) : NULL;
  int32_t n = 0;
  int rc = !hits || (rows_out && !rows) ? YRWI_E_NOMEM
                                        : yrwi_query_rows((yrwi_ctx*)(intptr_t)ctx, &q, hits, rows, &n, NULL);
  (*env)->ReleaseByteArrayElements(env, incl, ib, JNI_ABORT);
  (*env)->ReleaseByteArrayElements(env, excl, eb, JNI_ABORT);
  if (sx) (*env)->ReleaseByteArrayElements(env, siteExcludes, sx, JNI_ABORT);
  if (uh) (*env)->ReleaseByteArrayElements(env, urlHashes, uh, JNI_ABORT);
  (*env)->ReleaseStringUTFChars(env, lang, l);
  jbyteArray res = NULL;
  if (rc == 0) {
    if (flagCount) (*env)->SetIntArrayRegion(env, flagCount, 0, 32, (const jint*)fc);
    res = (*env)->NewByteArray(env, (jsize)(n * (jint)sizeof(yrwi_hit)));
    if (res) (*env)->SetByteArrayRegion(env, res, 0, (jsize)(n * (jint)sizeof(yrwi_hit)), (const jbyte*)hits);
    if (res && rows_out) {
      *rows_out = (*env)->NewByteArray(env, (jsize)(n * YRWI_ROW_BYTES));
      if (*rows_out) (*env)->SetByteArrayRegion(env, *rows_out, 0, (jsize)(n * YRWI_ROW_BYTES), (const jbyte*)rows);
      else res = NULL;
    }
  }
  free(hits);
  free(rows);
  return res;
}

JNIEXPORT jbyteArray JNICALL Java_net_yacy_kelondro_rwi_GpuRWI_queryFiltered(
    JNIEnv* env, jclass c, jlong ctx, jbyteArray incl, jint nincl, jbyteArray excl, jint nexcl, jint maxd, jint k,
    jintArray prof, jstring lang, jlong now, jbyteArray constraint, jboolean allOf, jint contentdom,
    jboolean strictDom, jstring modLang, jbyteArray site, jbyteArray altSite, jbyteArray siteExcludes,
    jbyteArray urlHashes, jboolean skipDoubleDom, jintArray flagCount) {
  return query_filtered(env, ctx, incl, nincl, excl, nexcl, maxd, k, prof, lang, now, constraint, allOf, contentdom,
                        strictDom, modLang, site, altSite, siteExcludes, urlHashes, skipDoubleDom, flagCount, NULL);
}

/* queryFiltered with the joined posting of every hit (yrwi_query_rows): byte[2][] = {the hits
 * (n * 24 bytes), their 40-byte WordReferenceRow rows (n * 40 bytes, hit order)}; NULL on failure. */
JNIEXPORT jobjectArray JNICALL Java_net_yacy_kelondro_rwi_GpuRWI_queryRows(
    JNIEnv* env, jclass c, jlong ctx, jbyteArray incl, jint nincl, jbyteArray excl, jint nexcl, jint maxd, jint k,
    jintArray prof, jstring lang, jlong now, jbyteArray constraint, jboolean allOf, jint contentdom,
    jboolean strictDom, jstring modLang, jbyteArray site, jbyteArray altSite, jbyteArray siteExcludes,
    jbyteArray urlHashes, jboolean skipDoubleDom, jintArray flagCount) {
  jbyteArray rows = NULL;
  jbyteArray hits = query_filtered(env, ctx, incl, nincl, excl, nexcl, maxd, k, prof, lang, now, constraint, allOf,
                                   contentdom, strictDom, modLang, site, altSite, siteExcludes, urlHashes,
                                   skipDoubleDom, flagCount, &rows);
  if (!hits || !rows) return NULL;
  jclass bytes = (*env)->FindClass(env, "[B");
  jobjectArray res = bytes ? (*env)->NewObjectArray(env, 2, bytes, NULL) : NULL;
  if (!res) return NULL;
  (*env)->SetObjectArrayElement(env, res, 0, hits);
  (*env)->SetObjectArrayElement(env, res, 1, rows);
  return res;
}

/* ---- search events (SearchEvent.addRWIs per arrival) ---- */
JNIEXPORT jlong JNICALL Java_net_yacy_kelondro_rwi_GpuRWI_eventOpen(JNIEnv* env, jclass c, jlong ctx, jintArray prof,
                                                                   jstring lang, jlong now, jint k, jlong maxPostings) {
  yrwi_profile p;
  to_profile(env, prof, &p);
  const char* l = (*env)->GetStringUTFChars(env, lang, NULL);
  yrwi_event* ev = NULL;
  int rc = yrwi_event_open((yrwi_ctx*)(intptr_t)ctx, &p, l, now, k, NULL, maxPostings, &ev);
  (*env)->ReleaseStringUTFChars(env, lang, l);
  return rc == 0 ? (jlong)(intptr_t)ev : 0;
}

/* GpuRWIStack's event: url set, rwiStack and doubleDomCache under the addRWIs constraints
 * (the same filter fields as queryFiltered; urlHashes seed the doublecheck set) */
JNIEXPORT jlong JNICALL Java_net_yacy_kelondro_rwi_GpuRWI_eventOpenFiltered(
    JNIEnv* env, jclass c, jlong ctx, jintArray prof, jstring lang, jlong now, jint k, jlong maxPostings,
    jbyteArray constraint, jboolean allOf, jint contentdom, jboolean strictDom, jstring modLang, jbyteArray site,
    jbyteArray altSite, jbyteArray siteExcludes, jbyteArray urlHashes) {
  yrwi_profile p;
  to_profile(env, prof, &p);
  yrwi_filter f;
  memset(&f, 0, sizeof(f));
  if (constraint) { (*env)->GetByteArrayRegion(env, constraint, 0, 4, (jbyte*)f.constraint); f.has_constraint = 1; }
  f.all_of_constraint = allOf;
  f.contentdom = contentdom;
  f.strict_contentdom = strictDom;
  if (modLang) {
    const char* ml = (*env)->GetStringUTFChars(env, modLang, NULL);
    strncpy(f.language, ml, sizeof(f.language) - 1);
    (*env)->ReleaseStringUTFChars(env, modLang, ml);
  }
  if (site) { (*env)->GetByteArrayRegion(env, site, 0, 6, (jbyte*)f.sitehash); f.has_sitehash = 1; }
  if (altSite) { (*env)->GetByteArrayRegion(env, altSite, 0, 6, (jbyte*)f.alt_sitehash); f.has_alt_sitehash = 1; }
  const jsize nsx = siteExcludes ? (*env)->GetArrayLength(env, siteExcludes) / 6 : 0;
  const jsize nuh = urlHashes ? (*env)->GetArrayLength(env, urlHashes) / 12 : 0;
  uint8_t* sx = nsx ? copy_in(env, siteExcludes, (int64_t)nsx * 6) : NULL;
  uint8_t* uh = nuh ? copy_in(env, urlHashes, (int64_t)nuh * 12) : NULL;
  f.siteexcludes = sx;
  f.nsiteexcludes = sx ? nsx : 0;
  f.urlhashes = uh;
  f.nurlhashes = uh ? nuh : 0;
  const char* l = (*env)->GetStringUTFChars(env, lang, NULL);
  yrwi_event* ev = NULL;
  int rc = yrwi_event_open((yrwi_ctx*)(intptr_t)ctx, &p, l, now, k, &f, maxPostings, &ev);
  (*env)->ReleaseStringUTFChars(env, lang, l);
  free(sx);
  free(uh);
  return rc == 0 ? (jlong)(intptr_t)ev : 0;
}

/* (arrival, row) of the admitted posting of each of n url hashes (yrwi_event_source): int[2n] */
JNIEXPORT jintArray JNICALL Java_net_yacy_kelondro_rwi_GpuRWI_eventSource(JNIEnv* env, jclass c, jlong ctx, jlong ev,
                                                                         jbyteArray urls, jint n) {
  uint8_t* u = copy_in(env, urls, (int64_t)n * 12);
  if (!u) return NULL;
  int32_t* a = (int32_t*)malloc(sizeof(int32_t) * 2 * (size_t)(n > 0 ? n : 1));
  int rc = a ? yrwi_event_source((yrwi_ctx*)(intptr_t)ctx, (yrwi_event*)(intptr_t)ev, u, n, a, a + (n > 0 ? n : 1))
             : YRWI_E_NOMEM;
  free(u);
  jintArray res = NULL;
  if (rc == 0) {
    jint* v = (jint*)malloc(sizeof(jint) * 2 * (size_t)(n > 0 ? n : 1));
    for (jint i = 0; v && i < n; i++) { v[2 * i] = a[i]; v[2 * i + 1] = a[(n > 0 ? n : 1) + i]; }
    res = (*env)->NewIntArray(env, 2 * n);
    if (v) (*env)->SetIntArrayRegion(env, res, 0, 2 * n, v);
    free(v);
  }
  free(a);
  return res;
}

/* SearchEvent.flagcount of an event (yrwi_event_result's info, no hits copied) */
JNIEXPORT jintArray JNICALL Java_net_yacy_kelondro_rwi_GpuRWI_eventFlagCount(JNIEnv* env, jclass c, jlong ctx,
                                                                            jlong ev) {
  yrwi_event_info info;
  int32_t n = 0;
  if (yrwi_event_result((yrwi_ctx*)(intptr_t)ctx, (yrwi_event*)(intptr_t)ev, NULL, 0, &n, &info) != 0) return NULL;
  jintArray res = (*env)->NewIntArray(env, 32);
  (*env)->SetIntArrayRegion(env, res, 0, 32, (const jint*)info.flagcount);
  return res;
}

/* GpuReferenceOrder's event: the ReferenceOrder state and host table only (yrwi_event_open_order) */
JNIEXPORT jlong JNICALL Java_net_yacy_kelondro_rwi_GpuRWI_eventOpenOrder(JNIEnv* env, jclass c, jlong ctx,
                                                                        jintArray prof, jstring lang, jlong now,
                                                                        jlong maxHosts) {
  yrwi_profile p;
  to_profile(env, prof, &p);
  const char* l = (*env)->GetStringUTFChars(env, lang, NULL);
  yrwi_event* ev = NULL;
  int rc = yrwi_event_open_order((yrwi_ctx*)(intptr_t)ctx, &p, l, now, maxHosts, &ev);
  (*env)->ReleaseStringUTFChars(env, lang, l);
  return rc == 0 ? (jlong)(intptr_t)ev : 0;
}

/* addRWIs(container, local): rows = RowSet.chunkcache bytes of the container in its order */
JNIEXPORT jint JNICALL Java_net_yacy_kelondro_rwi_GpuRWI_eventAdd(JNIEnv* env, jclass c, jlong ctx, jlong ev,
                                                                 jbyteArray rows, jint n, jboolean local) {
  yrwi_arrival a;
  memset(&a, 0, sizeof(a));
  uint8_t* p = copy_in(env, rows, (int64_t)n * 40);
  if (!p) return YRWI_E_ARG;
  a.ev = (yrwi_event*)(intptr_t)ev;
  a.rows40 = p;
  a.n = n;
  a.local = local ? 1 : 0;
  int rc = yrwi_event_add((yrwi_ctx*)(intptr_t)ctx, &a, 1);
  free(p);
  return rc;
}

/* addRWIs(termSearch.joined(), local = true) without the rows leaving the device
 * (yrwi_event_add_local): the joined and excluded container of the terms (sel: a url
 * selection or NULL) arrives at the event.  Returns m, the rows that arrived (0: an empty
 * container, the event is unchanged), or the (negative) error code. */
JNIEXPORT jlong JNICALL Java_net_yacy_kelondro_rwi_GpuRWI_eventAddLocal(JNIEnv* env, jclass c, jlong ctx, jlong ev,
                                                                       jbyteArray incl, jint nincl, jbyteArray excl,
                                                                       jint nexcl, jbyteArray sel, jint nsel,
                                                                       jint maxd, jlong now) {
  jbyte* ib = (*env)->GetByteArrayElements(env, incl, NULL);
  jbyte* eb = (*env)->GetByteArrayElements(env, excl, NULL);
  jbyte* sb = sel ? (*env)->GetByteArrayElements(env, sel, NULL) : NULL;
  yrwi_query_desc q;
  memset(&q, 0, sizeof(q));
  q.incl = (const uint8_t*)ib; q.nincl = nincl;
  q.excl = (const uint8_t*)eb; q.nexcl = nexcl;
  q.max_distance = maxd; q.k = 1; q.now_ms = now;
  q.urlselection = (const uint8_t*)sb; q.nurlselection = sb ? nsel : 0;
  yrwi_local_arrival a;
  memset(&a, 0, sizeof(a));
  a.ev = (yrwi_event*)(intptr_t)ev;
  a.q = &q;
  int rc = yrwi_event_add_local((yrwi_ctx*)(intptr_t)ctx, &a, 1, NULL);
  (*env)->ReleaseByteArrayElements(env, incl, ib, JNI_ABORT);
  (*env)->ReleaseByteArrayElements(env, excl, eb, JNI_ABORT);
  if (sb) (*env)->ReleaseByteArrayElements(env, sel, sb, JNI_ABORT);
  return rc == 0 ? (jlong)a.m : (jlong)rc;
}

/* The rows the event retained for n url hashes (yrwi_event_rows): n * 40 row bytes followed
 * by n found bytes (1: the url's admitted posting arrived through eventAddLocal, its row is
 * there; 0: 40 zero bytes) */
JNIEXPORT jbyteArray JNICALL Java_net_yacy_kelondro_rwi_GpuRWI_eventRows(JNIEnv* env, jclass c, jlong ctx, jlong ev,
                                                                        jbyteArray urls, jint n) {
  uint8_t* u = copy_in(env, urls, (int64_t)n * 12);
  if (!u) return NULL;
  const size_t nn = (size_t)(n > 0 ? n : 1);
  uint8_t* out = (uint8_t*)malloc(nn * 41);
  int rc = out ? yrwi_event_rows((yrwi_ctx*)(intptr_t)ctx, (yrwi_event*)(intptr_t)ev, u, n, out, out + (size_t)n * 40)
               : YRWI_E_NOMEM;
  free(u);
  jbyteArray res = NULL;
  if (rc == 0) {
    res = (*env)->NewByteArray(env, (jsize)(n * 41));
    (*env)->SetByteArrayRegion(env, res, 0, (jsize)(n * 41), (const jbyte*)out);
  }
  free(out);
  return res;
}

/* ReferenceOrder.normalizeWith + cardinal continuing the event's ReferenceOrder
 * (yrwi_event_order): one score per row of the container, in its order */
JNIEXPORT jlongArray JNICALL Java_net_yacy_kelondro_rwi_GpuRWI_eventOrder(JNIEnv* env, jclass c, jlong ctx, jlong ev,
                                                                         jbyteArray rows, jint n, jboolean local) {
  /* yrwi_event_order drains the context and synchronises with the GPU: the rows are
   * copied out of the Java heap first (no GC-blocking critical region around it) */
  uint8_t* p = copy_in(env, rows, (int64_t)n * 40);
  if (!p) return NULL;
  jlong* sc = (jlong*)malloc(sizeof(jlong) * (size_t)(n > 0 ? n : 1));
  if (!sc) { free(p); return NULL; }
  int rc = yrwi_event_order((yrwi_ctx*)(intptr_t)ctx, (yrwi_event*)(intptr_t)ev, p, n, local ? 1 : 0, (int64_t*)sc);
  free(p);
  jlongArray res = NULL;
  if (rc == 0) {
    res = (*env)->NewLongArray(env, n);
    (*env)->SetLongArrayRegion(env, res, 0, n, sc);
  }
  free(sc);
  return res;
}

/* ReferenceOrder.authority of n 6-byte host hashes against the event's host counts */
JNIEXPORT jintArray JNICALL Java_net_yacy_kelondro_rwi_GpuRWI_eventAuthority(JNIEnv* env, jclass c, jlong ctx,
                                                                            jlong ev, jbyteArray hosts6, jint n) {
  uint8_t* h = copy_in(env, hosts6, (int64_t)n * 6);
  if (!h) return NULL;
  jint* out = (jint*)malloc(sizeof(jint) * (size_t)(n > 0 ? n : 1));
  int rc = out ? yrwi_event_authority((yrwi_ctx*)(intptr_t)ctx, (yrwi_event*)(intptr_t)ev, h, n, (int32_t*)out)
               : YRWI_E_NOMEM;
  free(h);
  jintArray res = NULL;
  if (rc == 0) {
    res = (*env)->NewIntArray(env, n);
    (*env)->SetIntArrayRegion(env, res, 0, n, out);
  }
  free(out);
  return res;
}

/* rwiStack contents (yrwi_hit records) */
JNIEXPORT jbyteArray JNICALL Java_net_yacy_kelondro_rwi_GpuRWI_eventResult(JNIEnv* env, jclass c, jlong ctx, jlong ev,
                                                                          jint maxn) {
  yrwi_hit* hits = (yrwi_hit*)malloc(sizeof(yrwi_hit) * (size_t)(maxn > 0 ? maxn : 1));
  int32_t n = 0;
  int rc = yrwi_event_result((yrwi_ctx*)(intptr_t)ctx, (yrwi_event*)(intptr_t)ev, hits, maxn, &n, NULL);
  jbyteArray res = NULL;
  if (rc == 0) {
    res = (*env)->NewByteArray(env, (jsize)(n * (jint)sizeof(yrwi_hit)));
    (*env)->SetByteArrayRegion(env, res, 0, (jsize)(n * (jint)sizeof(yrwi_hit)), (const jbyte*)hits);
  }
  free(hits);
  return res;
}

/* pullOneRWI(skipDoubleDom) up to maxn times (SearchEvent.java:1297-1394): the
 * entries leave the event's rwiStack; yrwi_hit records in pull order */
JNIEXPORT jbyteArray JNICALL Java_net_yacy_kelondro_rwi_GpuRWI_eventPull(JNIEnv* env, jclass c, jlong ctx, jlong ev,
                                                                        jboolean skipDoubleDom, jint maxn) {
  yrwi_hit* hits = (yrwi_hit*)malloc(sizeof(yrwi_hit) * (size_t)(maxn > 0 ? maxn : 1));
  int32_t n = 0;
  int rc = yrwi_event_pull((yrwi_ctx*)(intptr_t)ctx, (yrwi_event*)(intptr_t)ev, skipDoubleDom ? 1 : 0, hits, maxn, &n);
  jbyteArray res = NULL;
  if (rc == 0) {
    res = (*env)->NewByteArray(env, (jsize)(n * (jint)sizeof(yrwi_hit)));
    (*env)->SetByteArrayRegion(env, res, 0, (jsize)(n * (jint)sizeof(yrwi_hit)), (const jbyte*)hits);
  }
  free(hits);
  return res;
}

JNIEXPORT void JNICALL Java_net_yacy_kelondro_rwi_GpuRWI_eventClose(JNIEnv* env, jclass c, jlong ctx, jlong ev) {
  yrwi_event_close((yrwi_ctx*)(intptr_t)ctx, (yrwi_event*)(intptr_t)ev);
}

/* ---- index abstracts: compressIndex per term (searchConjunction), one String each ---- */
JNIEXPORT jobjectArray JNICALL Java_net_yacy_kelondro_rwi_GpuRWI_indexAbstracts(JNIEnv* env, jclass c, jlong ctx,
                                                                               jbyteArray terms, jint nterms,
                                                                               jlong cap) {
  jbyte* tb = (*env)->GetByteArrayElements(env, terms, NULL);
  char* out = (char*)malloc((size_t)(cap > 0 ? cap : 1) + 1);
  int64_t* off = (int64_t*)calloc((size_t)nterms + 1, sizeof(int64_t));
  int32_t nout = 0;
  int rc = yrwi_index_abstracts((yrwi_ctx*)(intptr_t)ctx, (const uint8_t*)tb, nterms, NULL, out, cap, off, &nout);
  (*env)->ReleaseByteArrayElements(env, terms, tb, JNI_ABORT);
  jobjectArray res = NULL;
  if (rc == 0) {  /* abstract i = bytes [off[i], off[i+1]) (ASCII); none when a term has no list */
    res = (*env)->NewObjectArray(env, nout, (*env)->FindClass(env, "java/lang/String"), NULL);
    for (int32_t i = 0; i < nout; i++) {
      const char save = out[off[i + 1]];
      out[off[i + 1]] = 0;
      jstring s = (*env)->NewStringUTF(env, out + off[i]);
      out[off[i + 1]] = save;
      (*env)->SetObjectArrayElement(env, res, i, s);
      (*env)->DeleteLocalRef(env, s);
    }
  }
  free(out);
  free(off);
  return res;
}

/* ---- Index.size / Index.get of the GPU index (J1 sizes, TermSearch.inclusion) ---- */
JNIEXPORT jlongArray JNICALL Java_net_yacy_kelondro_rwi_GpuRWI_listSizes(JNIEnv* env, jclass c, jlong ctx,
                                                                        jbyteArray terms, jint nterms) {
  jbyte* tb = (*env)->GetByteArrayElements(env, terms, NULL);
  jlong* v = (jlong*)calloc((size_t)(nterms > 0 ? nterms : 1), sizeof(jlong));
  int rc = 0;
  for (jint i = 0; i < nterms && rc == 0; i++) {
    int64_t n = 0;
    rc = yrwi_list_size((yrwi_ctx*)(intptr_t)ctx, (const uint8_t*)tb + 12 * i, &n);
    v[i] = n;
  }
  (*env)->ReleaseByteArrayElements(env, terms, tb, JNI_ABORT);
  jlongArray res = NULL;
  if (rc == 0) {
    res = (*env)->NewLongArray(env, nterms);
    (*env)->SetLongArrayRegion(env, res, 0, nterms, v);
  }
  free(v);
  return res;
}

JNIEXPORT jbyteArray JNICALL Java_net_yacy_kelondro_rwi_GpuRWI_getList(JNIEnv* env, jclass c, jlong ctx,
                                                                      jbyteArray term) {
  yrwi_ctx* x = (yrwi_ctx*)(intptr_t)ctx;
  jbyte t[12];
  (*env)->GetByteArrayRegion(env, term, 0, 12, t);
  int64_t n = 0, m = 0;
  if (yrwi_list_size(x, (const uint8_t*)t, &n) != 0) return NULL;
  jbyteArray res = (*env)->NewByteArray(env, (jsize)(n * 40));
  if (n == 0) return res;
  /* the device copy lands in a native buffer first: no GC-blocking critical region
   * around the copy and its stream synchronisation.  yrwi_get_list drains the
   * context's batches; it must not run concurrently with yrwi_put_list (one
   * context per host thread, include/yrwi.h). */
  uint8_t* buf = (uint8_t*)malloc((size_t)n * 40);
  if (!buf) return NULL;
  int rc = yrwi_get_list(x, (const uint8_t*)t, buf, n, &m);
  if (rc == 0 && m == n) (*env)->SetByteArrayRegion(env, res, 0, (jsize)(n * 40), (const jbyte*)buf);
  free(buf);
  return rc == 0 && m == n ? res : NULL;
}

/* ---- Solr node stack: cardinal(URIMetadataNode); nodes = packed yrwi_node records ---- */
JNIEXPORT jlongArray JNICALL Java_net_yacy_kelondro_rwi_GpuRWI_scoreNodes(JNIEnv* env, jclass c, jlong ctx,
                                                                         jbyteArray nodes, jint n, jintArray prof,
                                                                         jstring lang, jint maxdomcount) {
  yrwi_profile p;
  to_profile(env, prof, &p);
  const char* l = (*env)->GetStringUTFChars(env, lang, NULL);
  jbyte* nb = (*env)->GetByteArrayElements(env, nodes, NULL);
  jlong* sc = (jlong*)malloc(sizeof(jlong) * (size_t)(n > 0 ? n : 1));
  int rc = yrwi_score_nodes((yrwi_ctx*)(intptr_t)ctx, (const yrwi_node*)nb, n, &p, l, maxdomcount, (int64_t*)sc);
  (*env)->ReleaseByteArrayElements(env, nodes, nb, JNI_ABORT);
  (*env)->ReleaseStringUTFChars(env, lang, l);
  jlongArray res = NULL;
  if (rc == 0) {
    res = (*env)->NewLongArray(env, n);
    (*env)->SetLongArrayRegion(env, res, 0, n, sc);
  }
  free(sc);
  return res;
}
