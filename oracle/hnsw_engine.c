/* ORACLE — test infrastructure ONLY (never linked into the product path).
 *
 * A self-contained, single-threaded, deterministic HNSW engine that restates
 * usearch 2.x's build and search algorithms in plain C, exported under the
 * same `ref_hnsw_*` C ABI as ref_hnsw_shim.cpp. oracle/hnsw.py loads it when
 * the usearch-backed shim (oracle/_ref/libref_hnsw.so, which needs the
 * usearch sources) has not been built, so the HNSW parity tests run from the
 * repository alone.
 *
 * Restated (studied, not copied) from usearch index.hpp:
 *   - level draw: floor(-ln(u) / ln(connectivity)), u uniform in (0, 1]
 *   - add: greedy descent (search_for_one_) from the entry point down to the
 *     node's level + 1, then per level a beam of width expansion_add
 *     (search_to_insert_), neighbor selection by the relative-neighborhood
 *     heuristic (refine_: keep a candidate only if it is closer to the new
 *     node than to every neighbor kept so far), at most `connectivity` links
 *     for the new node, reverse links up to `connectivity` (upper levels) or
 *     `connectivity_base` = 2 x connectivity (level 0), re-selected with the
 *     same heuristic on overflow
 *   - search: greedy descent to level 1, then the base-level beam
 *     (search_to_find_in_base_) exactly as oracle/hnsw.py's oracle_search
 *     states it, expansion max(ef, k); a key predicate gates insertion into
 *     `top` only
 *   - save: the index_dense serialization matrixone_amd.hnsw.
 *     load_usearch_index documents (f32 scalars, u64 keys, u32 slots)
 * Distances are f32: l2sq, ip = 1 - a.b, cos = 1 - a.b / (|a| |b|).
 */

#define _POSIX_C_SOURCE 200809L /* strdup */

#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define EXPORT __attribute__((visibility("default")))

typedef struct {
    float d;
    uint32_t s;
} cand_t;

typedef struct {
    cand_t* a;
    size_t n, cap;
} heap_t;

typedef struct {
    size_t dim;
    int metric;
    size_t M, M0, ef_add, ef_search;
    size_t n, cap;
    float* vecs;
    uint64_t* keys;
    int16_t* levels;
    uint32_t** nbr; /* per node: level-0 block (1 + M0 words) then one
                       (1 + M)-word block per upper level; word 0 = count */
    int max_level;
    uint32_t entry;
    uint32_t* visited;
    uint32_t epoch;
    uint64_t rng;
    heap_t next;
    cand_t* top;
    size_t top_cap;
} hnsw_t;

static void set_err(char** err, const char* msg) {
    if (err) *err = strdup(msg);
}

static int cand_less(cand_t a, cand_t b) {
    return a.d < b.d || (a.d == b.d && a.s < b.s);
}

static int heap_push(heap_t* h, cand_t c) {
    if (h->n == h->cap) {
        size_t nc = h->cap ? h->cap * 2 : 256;
        cand_t* na = (cand_t*)realloc(h->a, nc * sizeof(cand_t));
        if (!na) return -1;
        h->a = na;
        h->cap = nc;
    }
    size_t i = h->n++;
    while (i > 0) {
        size_t p = (i - 1) / 2;
        if (!cand_less(c, h->a[p])) break;
        h->a[i] = h->a[p];
        i = p;
    }
    h->a[i] = c;
    return 0;
}

static void heap_pop(heap_t* h) {
    cand_t last = h->a[--h->n];
    size_t i = 0;
    for (;;) {
        size_t l = 2 * i + 1, r = l + 1, m;
        if (l >= h->n) break;
        m = (r < h->n && cand_less(h->a[r], h->a[l])) ? r : l;
        if (!cand_less(h->a[m], last)) break;
        h->a[i] = h->a[m];
        i = m;
    }
    if (h->n) h->a[i] = last;
}

static float dist_vv(const hnsw_t* h, const float* a, const float* b) {
    const size_t d = h->dim;
    if (h->metric == 0) {
        float s = 0.0f;
        for (size_t i = 0; i < d; ++i) {
            float t = a[i] - b[i];
            s += t * t;
        }
        return s;
    }
    float ab = 0.0f;
    for (size_t i = 0; i < d; ++i) ab += a[i] * b[i];
    if (h->metric == 1) return 1.0f - ab;
    float a2 = 0.0f, b2 = 0.0f;
    for (size_t i = 0; i < d; ++i) {
        a2 += a[i] * a[i];
        b2 += b[i] * b[i];
    }
    if (a2 == 0.0f || b2 == 0.0f) return 1.0f;
    return 1.0f - ab / (sqrtf(a2) * sqrtf(b2));
}

static const float* vec_of(const hnsw_t* h, uint32_t s) {
    return h->vecs + (size_t)s * h->dim;
}

static uint32_t* nb_block(const hnsw_t* h, uint32_t s, int level) {
    return h->nbr[s] +
           (level == 0 ? 0 : (h->M0 + 1) + (size_t)(level - 1) * (h->M + 1));
}

static int passes(const hnsw_t* h, uint32_t s, const uint32_t* bits,
                  uint64_t nbits) {
    if (!bits) return 1;
    uint64_t key = h->keys[s];
    if (key >= nbits) return 0;
    return (bits[key >> 5] >> (key & 31)) & 1u;
}

static int ensure_top(hnsw_t* h, size_t ef) {
    if (ef <= h->top_cap) return 0;
    cand_t* nt = (cand_t*)realloc(h->top, ef * sizeof(cand_t));
    if (!nt) return -1;
    h->top = nt;
    h->top_cap = ef;
    return 0;
}

/* Greedy descent over levels from_level .. to_level + 1 (search_for_one_). */
static uint32_t descend(const hnsw_t* h, const float* q, int from_level,
                        int to_level, float* out_d) {
    uint32_t closest = h->entry;
    float closest_d = dist_vv(h, vec_of(h, closest), q);
    for (int level = from_level; level > to_level; --level) {
        int changed = 1;
        while (changed) {
            changed = 0;
            const uint32_t* blk = nb_block(h, closest, level);
            const uint32_t cnt = blk[0];
            for (uint32_t i = 0; i < cnt; ++i) {
                float d = dist_vv(h, vec_of(h, blk[1 + i]), q);
                if (d < closest_d) {
                    closest_d = d;
                    closest = blk[1 + i];
                    changed = 1;
                }
            }
        }
    }
    *out_d = closest_d;
    return closest;
}

/* Beam of width ef on one level; h->top holds the result ascending.
 * Returns the result count, or -1 when out of memory. */
static int64_t beam(hnsw_t* h, const float* q, uint32_t start, float start_d,
                    int level, size_t ef, const uint32_t* bits,
                    uint64_t nbits) {
    if (ensure_top(h, ef)) return -1;
    if (++h->epoch == 0) {
        memset(h->visited, 0, h->cap * sizeof(uint32_t));
        h->epoch = 1;
    }
    cand_t* top = h->top;
    size_t ntop = 0;
    h->next.n = 0;
    h->visited[start] = h->epoch;
    if (heap_push(&h->next, (cand_t){start_d, start})) return -1;
    float radius = start_d;
    if (passes(h, start, bits, nbits)) top[ntop++] = (cand_t){start_d, start};
    while (h->next.n) {
        cand_t c = h->next.a[0];
        if (c.d > radius && ntop == ef) break;
        heap_pop(&h->next);
        const uint32_t* blk = nb_block(h, c.s, level);
        const uint32_t cnt = blk[0];
        for (uint32_t i = 0; i < cnt; ++i) {
            const uint32_t nb = blk[1 + i];
            if (h->visited[nb] == h->epoch) continue;
            h->visited[nb] = h->epoch;
            const float d = dist_vv(h, vec_of(h, nb), q);
            if (ntop < ef || d < radius) {
                if (heap_push(&h->next, (cand_t){d, nb})) return -1;
                if (passes(h, nb, bits, nbits)) {
                    if (ntop == ef) --ntop; /* the farthest one leaves */
                    size_t j = ntop++;
                    while (j > 0 && top[j - 1].d > d) {
                        top[j] = top[j - 1];
                        --j;
                    }
                    top[j] = (cand_t){d, nb};
                    radius = top[ntop - 1].d;
                }
            }
        }
    }
    return (int64_t)ntop;
}

/* Neighbor selection (refine_): `c` ascending by distance to the node at
 * `self`; keeps at most maxn, written to out. Returns the kept count. */
static size_t refine(const hnsw_t* h, const cand_t* c, size_t n, size_t maxn,
                     uint32_t* out) {
    size_t kept = 0;
    for (size_t i = 0; i < n && kept < maxn; ++i) {
        int good = 1;
        for (size_t j = 0; j < kept; ++j) {
            if (dist_vv(h, vec_of(h, c[i].s), vec_of(h, out[j])) < c[i].d) {
                good = 0;
                break;
            }
        }
        if (good) out[kept++] = c[i].s;
    }
    return kept;
}

static int cand_cmp(const void* a, const void* b) {
    const cand_t x = *(const cand_t*)a, y = *(const cand_t*)b;
    return cand_less(x, y) ? -1 : cand_less(y, x) ? 1 : 0;
}

static double next_uniform(hnsw_t* h) { /* splitmix64 -> (0, 1] */
    uint64_t z = (h->rng += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return ((double)(z >> 11) + 1.0) * (1.0 / 9007199254740992.0);
}

static int reserve(hnsw_t* h, size_t cap) {
    if (cap <= h->cap) return 0;
    float* v = (float*)realloc(h->vecs, cap * h->dim * sizeof(float));
    if (v) h->vecs = v;
    uint64_t* k = (uint64_t*)realloc(h->keys, cap * sizeof(uint64_t));
    if (k) h->keys = k;
    int16_t* l = (int16_t*)realloc(h->levels, cap * sizeof(int16_t));
    if (l) h->levels = l;
    uint32_t** nb = (uint32_t**)realloc(h->nbr, cap * sizeof(uint32_t*));
    if (nb) h->nbr = nb;
    uint32_t* vis = (uint32_t*)realloc(h->visited, cap * sizeof(uint32_t));
    if (vis) h->visited = vis;
    if (!v || !k || !l || !nb || !vis) return -1;
    memset(h->visited + h->cap, 0, (cap - h->cap) * sizeof(uint32_t));
    h->cap = cap;
    return 0;
}

static int add_one(hnsw_t* h, uint64_t key, const float* vec) {
    if (h->n == h->cap && reserve(h, h->cap ? h->cap * 2 : 1024)) return -1;
    int level = (int)floor(-log(next_uniform(h)) / log((double)h->M));
    if (level > 30) level = 30;
    const uint32_t s = (uint32_t)h->n;
    const size_t words = (h->M0 + 1) + (size_t)level * (h->M + 1);
    uint32_t* blk = (uint32_t*)calloc(words, sizeof(uint32_t));
    if (!blk) return -1;
    memcpy(h->vecs + (size_t)s * h->dim, vec, h->dim * sizeof(float));
    h->keys[s] = key;
    h->levels[s] = (int16_t)level;
    h->nbr[s] = blk;
    h->n++;
    if (s == 0) {
        h->entry = 0;
        h->max_level = level;
        return 0;
    }
    float closest_d;
    uint32_t closest = descend(h, vec, h->max_level, level, &closest_d);
    const size_t scratch_n = h->M0 + 2;
    cand_t* scratch = (cand_t*)malloc(scratch_n * sizeof(cand_t));
    uint32_t* sel = (uint32_t*)malloc(scratch_n * sizeof(uint32_t));
    if (!scratch || !sel) {
        free(scratch);
        free(sel);
        return -1;
    }
    int rc = 0;
    for (int l = level < h->max_level ? level : h->max_level; l >= 0; --l) {
        int64_t ntop = beam(h, vec, closest, closest_d, l, h->ef_add, NULL, 0);
        if (ntop < 0) {
            rc = -1;
            break;
        }
        closest = h->top[0].s;
        closest_d = h->top[0].d;
        uint32_t* mine = nb_block(h, s, l);
        mine[0] = (uint32_t)refine(h, h->top, (size_t)ntop, h->M, mine + 1);
        const size_t lcap = l == 0 ? h->M0 : h->M;
        for (uint32_t i = 0; i < mine[0]; ++i) {
            const uint32_t r = mine[1 + i];
            uint32_t* rb = nb_block(h, r, l);
            if (rb[0] < lcap) {
                rb[1 + rb[0]++] = s;
                continue;
            }
            size_t nc = 0;
            for (uint32_t j = 0; j < rb[0]; ++j)
                scratch[nc++] = (cand_t){
                    dist_vv(h, vec_of(h, rb[1 + j]), vec_of(h, r)), rb[1 + j]};
            scratch[nc++] = (cand_t){dist_vv(h, vec, vec_of(h, r)), s};
            qsort(scratch, nc, sizeof(cand_t), cand_cmp);
            const size_t kept = refine(h, scratch, nc, lcap, sel);
            rb[0] = (uint32_t)kept;
            memcpy(rb + 1, sel, kept * sizeof(uint32_t));
        }
    }
    free(scratch);
    free(sel);
    if (rc == 0 && level > h->max_level) {
        h->entry = s;
        h->max_level = level;
    }
    return rc;
}

static size_t search_one(hnsw_t* h, const float* query, size_t ef, size_t k,
                         const uint32_t* bits, uint64_t nbits,
                         uint64_t* out_keys, float* out_dists, char** err) {
    if (h->n == 0 || k == 0) return 0;
    if (ef < k) ef = k;
    float d0;
    const uint32_t start = descend(h, query, h->max_level, 0, &d0);
    int64_t ntop = beam(h, query, start, d0, 0, ef, bits, nbits);
    if (ntop < 0) {
        set_err(err, "out of memory");
        return 0;
    }
    size_t cnt = (size_t)ntop < k ? (size_t)ntop : k;
    for (size_t i = 0; i < cnt; ++i) {
        out_keys[i] = h->keys[h->top[i].s];
        out_dists[i] = h->top[i].d;
    }
    return cnt;
}

EXPORT void* ref_hnsw_create(size_t dim, int metric, size_t connectivity,
                             size_t expansion_add, size_t expansion_search,
                             size_t capacity, size_t threads, char** err) {
    (void)threads;
    if (dim == 0 || connectivity < 2 || metric < 0 || metric > 2) {
        set_err(err, "bad parameters");
        return NULL;
    }
    hnsw_t* h = (hnsw_t*)calloc(1, sizeof(hnsw_t));
    if (!h) {
        set_err(err, "out of memory");
        return NULL;
    }
    h->dim = dim;
    h->metric = metric;
    h->M = connectivity;
    h->M0 = connectivity * 2;
    h->ef_add = expansion_add ? expansion_add : 128;
    h->ef_search = expansion_search ? expansion_search : 64;
    h->rng = 0x243F6A8885A308D3ull;
    if (reserve(h, capacity ? capacity : 1024)) {
        set_err(err, "reserve failed");
        free(h);
        return NULL;
    }
    return h;
}

EXPORT int ref_hnsw_add_batch(void* hp, const uint64_t* keys,
                              const float* vecs, size_t n, size_t dim,
                              size_t threads, char** err) {
    (void)threads; /* inserts run in order: the graph is reproducible */
    hnsw_t* h = (hnsw_t*)hp;
    if (dim != h->dim) {
        set_err(err, "dimension mismatch");
        return -1;
    }
    for (size_t i = 0; i < n; ++i)
        if (add_one(h, keys[i], vecs + i * dim)) {
            set_err(err, "out of memory");
            return -1;
        }
    return 0;
}

EXPORT size_t ref_hnsw_search(void* hp, const float* query, size_t ef,
                              size_t k, uint64_t* out_keys, float* out_dists,
                              char** err) {
    return search_one((hnsw_t*)hp, query, ef, k, NULL, 0, out_keys, out_dists,
                      err);
}

EXPORT size_t ref_hnsw_search_filtered(void* hp, const float* query, size_t ef,
                                       size_t k, const uint32_t* key_bits,
                                       uint64_t nbits, uint64_t* out_keys,
                                       float* out_dists, char** err) {
    return search_one((hnsw_t*)hp, query, ef, k, key_bits, nbits, out_keys,
                      out_dists, err);
}

EXPORT size_t ref_hnsw_size(void* hp) { return ((hnsw_t*)hp)->n; }

EXPORT int ref_hnsw_max_level(void* hp) { return ((hnsw_t*)hp)->max_level; }

EXPORT uint64_t ref_hnsw_entry_slot(void* hp) { return ((hnsw_t*)hp)->entry; }

EXPORT uint64_t ref_hnsw_key_of_slot(void* hp, uint32_t slot) {
    return ((hnsw_t*)hp)->keys[slot];
}

EXPORT int ref_hnsw_node_level(void* hp, uint32_t slot) {
    return ((hnsw_t*)hp)->levels[slot];
}

EXPORT size_t ref_hnsw_neighbors(void* hp, uint32_t slot, int level,
                                 uint32_t* out, size_t cap) {
    hnsw_t* h = (hnsw_t*)hp;
    if (level > h->levels[slot]) return 0;
    const uint32_t* blk = nb_block(h, slot, level);
    for (size_t i = 0; i < blk[0] && i < cap; ++i) out[i] = blk[1 + i];
    return blk[0];
}

EXPORT int ref_hnsw_get_vector(void* hp, uint32_t slot, float* out,
                               size_t dim) {
    hnsw_t* h = (hnsw_t*)hp;
    if (slot >= h->n || dim != h->dim) return -1;
    memcpy(out, vec_of(h, slot), dim * sizeof(float));
    return 0;
}

EXPORT int64_t ref_hnsw_export_bulk(void* hp, size_t dim, int32_t* levels,
                                    uint64_t* keys, float* vecs,
                                    int64_t* l0_offs, uint32_t* l0_nbrs,
                                    int64_t l0_cap) {
    hnsw_t* h = (hnsw_t*)hp;
    int64_t off = 0;
    for (size_t s = 0; s < h->n; ++s) {
        levels[s] = h->levels[s];
        keys[s] = h->keys[s];
        memcpy(vecs + s * dim, vec_of(h, (uint32_t)s), dim * sizeof(float));
        l0_offs[s] = off;
        const uint32_t* blk = nb_block(h, (uint32_t)s, 0);
        if (off + (int64_t)blk[0] > l0_cap) return -1;
        for (uint32_t i = 0; i < blk[0]; ++i) l0_nbrs[off++] = blk[1 + i];
    }
    l0_offs[h->n] = off;
    return off;
}

EXPORT int64_t ref_hnsw_export_level(void* hp, int level, int64_t* offs,
                                     uint32_t* nbrs, int64_t cap) {
    hnsw_t* h = (hnsw_t*)hp;
    int64_t off = 0;
    for (size_t s = 0; s < h->n; ++s) {
        offs[s] = off;
        if (h->levels[s] >= level) {
            const uint32_t* blk = nb_block(h, (uint32_t)s, level);
            if (off + (int64_t)blk[0] > cap) return -1;
            for (uint32_t i = 0; i < blk[0]; ++i) nbrs[off++] = blk[1 + i];
        }
    }
    offs[h->n] = off;
    return off;
}

EXPORT int ref_hnsw_save(void* hp, const char* path, char** err) {
    hnsw_t* h = (hnsw_t*)hp;
    FILE* f = fopen(path, "wb");
    if (!f) {
        set_err(err, "cannot open file for writing");
        return -1;
    }
    const uint32_t rows = (uint32_t)h->n;
    const uint32_t bpv = (uint32_t)(h->dim * sizeof(float));
    int ok = fwrite(&rows, 4, 1, f) == 1 && fwrite(&bpv, 4, 1, f) == 1;
    if (ok && h->n)
        ok = fwrite(h->vecs, bpv, h->n, f) == h->n;
    uint8_t head[64];
    memset(head, 0, sizeof head);
    memcpy(head, "usearch", 7);
    const uint16_t version[3] = {2, 25, 3};
    memcpy(head + 7, version, 6);
    head[13] = (uint8_t)"eic"[h->metric]; /* metric kind: l2sq / ip / cos */
    head[14] = 11;                         /* scalar kind f32 */
    head[15] = 14;                         /* key kind u64 */
    head[16] = 15;                         /* compressed slot kind u32 */
    const uint64_t present = h->n, deleted = 0, dims = h->dim;
    memcpy(head + 17, &present, 8);
    memcpy(head + 25, &deleted, 8);
    memcpy(head + 33, &dims, 8);
    ok = ok && fwrite(head, 64, 1, f) == 1;
    const uint64_t hdr[5] = {h->n, h->M, h->M0, (uint64_t)h->max_level,
                             h->entry};
    ok = ok && fwrite(hdr, 8, 5, f) == 5;
    if (ok && h->n) ok = fwrite(h->levels, 2, h->n, f) == h->n;
    for (size_t s = 0; ok && s < h->n; ++s) {
        const size_t words =
            (h->M0 + 1) + (size_t)h->levels[s] * (h->M + 1);
        ok = fwrite(&h->keys[s], 8, 1, f) == 1 &&
             fwrite(&h->levels[s], 2, 1, f) == 1 &&
             fwrite(h->nbr[s], 4, words, f) == words;
    }
    if (fclose(f) != 0) ok = 0;
    if (!ok) {
        set_err(err, "short write");
        return -1;
    }
    return 0;
}

EXPORT void* ref_hnsw_load(const char* path, char** err) {
    (void)path;
    set_err(err, "load is not supported by the in-repository engine");
    return NULL;
}

EXPORT void ref_hnsw_free(void* hp) {
    hnsw_t* h = (hnsw_t*)hp;
    if (!h) return;
    for (size_t s = 0; s < h->n; ++s) free(h->nbr[s]);
    free(h->nbr);
    free(h->vecs);
    free(h->keys);
    free(h->levels);
    free(h->visited);
    free(h->next.a);
    free(h->top);
    free(h);
}
