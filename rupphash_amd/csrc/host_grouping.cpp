// host_grouping.cpp -- host-side halves of the reference's groupers (the parts that are serial in
// the reference too) and its scalar integer helpers.
//   union-find + group listing      /root/reference/src/scanner.rs:1781-1817
//   greedy star clustering          /root/reference/src/hamminghash.rs:245-268
//   HammingHash scalar functions    /root/reference/src/hamminghash.rs:23-63
//   64-bit pHash bit operations     /root/reference/src/phash.rs:137-255
#include <algorithm>
#include <cstring>
#include <vector>

#include "rph_internal.h"

// ---------------------------------------------------------------------------------------------
// scalar helpers
// ---------------------------------------------------------------------------------------------
extern "C" uint32_t rph_hamming_distance256(const uint8_t *a, const uint8_t *b)
{
    uint64_t x[4], y[4];
    std::memcpy(x, a, 32);
    std::memcpy(y, b, 32);
    return (uint32_t)(__builtin_popcountll(x[0] ^ y[0]) + __builtin_popcountll(x[1] ^ y[1]) +
                      __builtin_popcountll(x[2] ^ y[2]) + __builtin_popcountll(x[3] ^ y[3]));
}
extern "C" uint32_t rph_hamming_distance64(uint64_t a, uint64_t b) { return (uint32_t)__builtin_popcountll(a ^ b); }
extern "C" uint16_t rph_get_chunk256(const uint8_t *h, uint32_t k)
{
    return (uint16_t)(h[2 * k] | ((uint16_t)h[2 * k + 1] << 8));  // u16::from_le_bytes, hamminghash.rs:50-53
}
extern "C" uint16_t rph_get_chunk64(uint64_t h, uint32_t k) { return (uint16_t)((h >> (k * 8)) & 0xFF); }
extern "C" int rph_is_low_pdq_quality(int32_t q) { return q >= 0 && q < RPH_PDQ_MIN_QUALITY; }

extern "C" void rph_pdq_target_dimensions(uint32_t w, uint32_t h, uint32_t max_dim, uint32_t *nw, uint32_t *nh)
{
    // calculate_target_dimensions, pdqhash.rs:224-235
    if (w == 0 || h == 0) {
        *nw = std::max(w, 1u);
        *nh = std::max(h, 1u);
    } else if (w > h) {
        *nw = max_dim;
        *nh = (uint32_t)std::max<uint64_t>((uint64_t)h * max_dim / w, 1);
    } else {
        *nw = (uint32_t)std::max<uint64_t>((uint64_t)w * max_dim / h, 1);
        *nh = max_dim;
    }
}

// ---- pHash: bit i (from the MSB) is DCT cell (y = i / 8, x = i % 8); phash.rs:150-230 ----
static inline uint64_t remap(uint64_t hash, bool transpose, int flip_rule)
{
    uint64_t out = 0;
    for (int y = 0; y < 8; y++)
        for (int x = 0; x < 8; x++) {
            const int dx = transpose ? y : x, dy = transpose ? x : y;
            uint64_t bit = (hash >> (63 - (8 * y + x))) & 1;
            bool flip = false;
            switch (flip_rule) {
                case 0: flip = (dx & 1) != 0; break;         // odd destination column
                case 1: flip = (dy & 1) != 0; break;         // odd destination row
                case 2: flip = ((dx + dy) & 1) != 0; break;  // odd x + y
            }
            out |= (bit ^ (flip ? 1u : 0u)) << (63 - (8 * dy + dx));
        }
    return out;
}
extern "C" uint64_t rph_phash_rotate_90(uint64_t h) { return remap(h, true, 0); }
extern "C" uint64_t rph_phash_rotate_180(uint64_t h) { return remap(h, false, 2); }
extern "C" uint64_t rph_phash_rotate_270(uint64_t h) { return remap(h, true, 1); }
extern "C" uint64_t rph_phash_flip_horizontal(uint64_t h) { return remap(h, false, 0); }
extern "C" uint64_t rph_phash_rotation_invariant(uint64_t h)
{
    return std::min(std::min(h, rph_phash_rotate_90(h)), std::min(rph_phash_rotate_180(h), rph_phash_rotate_270(h)));
}
extern "C" void rph_phash_dihedral(uint64_t h, uint64_t out[8])
{
    const uint64_t f = rph_phash_flip_horizontal(h);
    out[0] = h;
    out[1] = rph_phash_rotate_90(h);
    out[2] = rph_phash_rotate_180(h);
    out[3] = rph_phash_rotate_270(h);
    out[4] = f;
    out[5] = rph_phash_rotate_90(f);
    out[6] = rph_phash_rotate_180(f);
    out[7] = rph_phash_rotate_270(f);
}

// ---------------------------------------------------------------------------------------------
// union-find (scanner.rs:1781-1817)
// ---------------------------------------------------------------------------------------------
namespace {
inline uint32_t uf_find(std::vector<uint32_t> &parent, uint32_t i)
{
    uint32_t root = i;
    while (root != parent[root]) root = parent[root];
    while (i != root) {
        const uint32_t next = parent[i];
        parent[i] = root;
        i = next;
    }
    return root;
}

// union of the edges' ends (scanner.rs:1797-1803)
int uf_apply_edges(std::vector<uint32_t> &parent, const rph_edge *edges, uint64_t n_edges)
{
    const uint64_t n = parent.size();
    for (uint64_t e = 0; e < n_edges; e++) {
        if (edges[e].i >= n || edges[e].j >= n) {
            rph_set_error("union-find: edge %llu references file %u/%u outside n=%llu", (unsigned long long)e, edges[e].i,
                          edges[e].j, (unsigned long long)n);
            return RPH_ERR_INVALID_ARG;
        }
        const uint32_t ri = uf_find(parent, edges[e].i), rj = uf_find(parent, edges[e].j);
        if (ri != rj) parent[ri] = rj;
    }
    return RPH_OK;
}

// Components with more than one member; members ascending (the reference pushes i in 0..n order,
// scanner.rs:1810-1814), groups ordered by their first member.
void uf_list_groups(std::vector<uint32_t> &parent, uint32_t *members, uint32_t *offsets, uint32_t *n_groups_out)
{
    const uint64_t n = parent.size();
    std::vector<uint32_t> root(n), count(n, 0), slot(n, UINT32_MAX);
    for (uint64_t i = 0; i < n; i++) {
        root[i] = uf_find(parent, (uint32_t)i);
        count[root[i]]++;
    }
    uint32_t ng = 0, total = 0;
    offsets[0] = 0;
    for (uint64_t i = 0; i < n; i++) {
        const uint32_t r = root[i];
        if (count[r] > 1 && slot[r] == UINT32_MAX) {
            slot[r] = ng++;
            total += count[r];
            offsets[ng] = total;
        }
    }
    std::vector<uint32_t> fill(ng, 0);
    for (uint64_t i = 0; i < n; i++) {
        const uint32_t r = root[i];
        if (count[r] > 1) {
            const uint32_t g = slot[r];
            members[offsets[g] + fill[g]++] = (uint32_t)i;
        }
    }
    *n_groups_out = ng;
}
}  // namespace

int rph_host_union_find(const rph_edge *edges, uint64_t n_edges, uint64_t n, uint32_t *members, uint32_t *offsets,
                        uint32_t *n_groups_out)
{
    std::vector<uint32_t> parent(n);
    for (uint64_t i = 0; i < n; i++) parent[i] = (uint32_t)i;
    RPH_TRY(uf_apply_edges(parent, edges, n_edges));
    uf_list_groups(parent, members, offsets, n_groups_out);
    return RPH_OK;
}

// The components an earlier call reported are joined first, then the new edges: connected components do not depend on the order of
// the unions, so the result is that of one union-find over the old edges and the new ones.  The old groups come from a file the
// caller kept between runs: every index is checked before it is used.
int rph_host_union_find_append(const uint32_t *old_members, const uint32_t *old_offsets, uint32_t n_old_groups, const rph_edge *edges,
                               uint64_t n_edges, uint64_t n, uint32_t *members, uint32_t *offsets, uint32_t *n_groups_out)
{
    if (n > 0xFFFFFFFFull) {
        rph_set_error("union-find: %llu files, at most 2^32 - 1", (unsigned long long)n);
        return RPH_ERR_INVALID_ARG;
    }
    if (n_old_groups && old_offsets[0] != 0) {
        rph_set_error("union-find: old offsets start at %u, not 0", old_offsets[0]);
        return RPH_ERR_INVALID_ARG;
    }
    for (uint32_t g = 0; g < n_old_groups; g++)
        if (old_offsets[g + 1] < old_offsets[g] || old_offsets[g + 1] > n) {  // (distinct members: no more than n of them)
            rph_set_error("union-find: old offsets are not ascending within n=%llu at group %u", (unsigned long long)n, g);
            return RPH_ERR_INVALID_ARG;
        }
    std::vector<uint32_t> parent(n);
    for (uint64_t i = 0; i < n; i++) parent[i] = (uint32_t)i;
    std::vector<uint8_t> seen(n, 0);
    for (uint32_t g = 0; g < n_old_groups; g++)
        for (uint32_t t = old_offsets[g]; t < old_offsets[g + 1]; t++) {
            const uint32_t m = old_members[t];
            if (m >= n || seen[m]) {
                rph_set_error("union-find: old group %u lists file %u %s", g, m, m >= n ? "outside n" : "twice");
                return RPH_ERR_INVALID_ARG;
            }
            seen[m] = 1;
            if (t > old_offsets[g]) parent[uf_find(parent, m)] = uf_find(parent, old_members[old_offsets[g]]);
        }
    RPH_TRY(uf_apply_edges(parent, edges, n_edges));
    uf_list_groups(parent, members, offsets, n_groups_out);
    return RPH_OK;
}

// ---------------------------------------------------------------------------------------------
// find_groups from an exhaustive edge list (hamminghash.rs:191-271)
//
// The reference's adjacency of query i is the list of candidates in first-seen order of its probe
// loop: chunk k ascending; within a chunk the exact bucket, then the flips of bit 0..15; within a
// bucket ascending id (CSR fill order).  A candidate is first seen at the smallest k whose 16-bit
// difference has popcount <= tolerance; the sweep kernel stored (k, slot) in edge.flags, and the
// key is symmetric in (i, j).  Pairs that no probe reaches are not adjacent.
// ---------------------------------------------------------------------------------------------
int rph_host_find_groups(const rph_edge *edges, uint64_t n_edges, uint64_t n, uint32_t *members, uint32_t *offsets,
                         uint32_t *n_groups_out)
{
    std::vector<uint64_t> deg(n + 1, 0);
    for (uint64_t e = 0; e < n_edges; e++) {
        if (!(edges[e].flags & RPH_EDGE_MIH_R1)) continue;
        if (edges[e].i >= n || edges[e].j >= n) {
            rph_set_error("find_groups: edge %llu outside n", (unsigned long long)e);
            return RPH_ERR_INVALID_ARG;
        }
        deg[edges[e].i + 1]++;
        deg[edges[e].j + 1]++;
    }
    for (uint64_t i = 0; i < n; i++) deg[i + 1] += deg[i];
    struct Nb {
        uint32_t key;  // (k << 5 | slot)
        uint32_t id;
    };
    std::vector<Nb> adj(deg[n]);
    std::vector<uint64_t> cur(deg.begin(), deg.end() - 1);
    for (uint64_t e = 0; e < n_edges; e++) {
        if (!(edges[e].flags & RPH_EDGE_MIH_R1)) continue;
        const uint32_t key = edges[e].flags & RPH_EDGE_PROBE_MASK;
        adj[cur[edges[e].i]++] = {key, edges[e].j};
        adj[cur[edges[e].j]++] = {key, edges[e].i};
    }
    for (uint64_t i = 0; i < n; i++)
        std::sort(adj.begin() + deg[i], adj.begin() + deg[i + 1],
                  [](const Nb &a, const Nb &b) { return a.key != b.key ? a.key < b.key : a.id < b.id; });

    // greedy clustering, hamminghash.rs:245-268
    std::vector<uint8_t> visited(n, 0);
    uint32_t ng = 0, total = 0;
    offsets[0] = 0;
    for (uint64_t i = 0; i < n; i++) {
        if (visited[i] || deg[i + 1] == deg[i]) continue;
        const uint32_t start = total;
        members[total++] = (uint32_t)i;
        visited[i] = 1;
        for (uint64_t t = deg[i]; t < deg[i + 1]; t++) {
            const uint32_t nb = adj[t].id;
            if (!visited[nb]) {
                visited[nb] = 1;
                members[total++] = nb;
            }
        }
        if (total - start > 1)
            offsets[++ng] = total;
        else
            total = start;
    }
    *n_groups_out = ng;
    return RPH_OK;
}

// ---------------------------------------------------------------------------------------------
// max_dist of every group (scanner.rs:1986-2022, :2214-2241): the rule on the host
// ---------------------------------------------------------------------------------------------
int rph_host_group_lists_check(const char *who, const uint8_t *hashes32, uint64_t n, const uint32_t *members, const uint32_t *offsets, uint32_t n_groups,
                               const uint32_t *pivots, const uint32_t *max_dist_out)
{
    const auto refuse = [&](const char *what) {
        rph_set_error("%s: %s", who, what);
        return RPH_ERR_INVALID_ARG;
    };
    if (n_groups == 0) return RPH_OK;
    if (!offsets || !max_dist_out || (!hashes32 && n)) return refuse("null argument");
    if (n >= RPH_NO_PIVOT) return refuse("at most 2^32 - 2 files");
    if (offsets[0] != 0) return refuse("offsets do not start at 0");
    for (uint32_t g = 0; g < n_groups; g++)
        if (offsets[g + 1] < offsets[g]) return refuse("offsets do not ascend");
    const uint32_t total = offsets[n_groups];
    if (total && !members) return refuse("null argument");
    for (uint32_t t = 0; t < total; t++)
        if (members[t] >= n) return refuse("a member is not below n");
    for (uint32_t g = 0; g < n_groups && pivots; g++)
        if (pivots[g] != RPH_NO_PIVOT && pivots[g] >= n) return refuse("a pivot is neither below n nor RPH_NO_PIVOT");
    return RPH_OK;
}

uint32_t rph_host_default_pivot(const uint32_t *members, const uint32_t *offsets, uint32_t g, const float *coeffs, const uint8_t *has_features)
{
    if (offsets[g] == offsets[g + 1]) return RPH_NO_PIVOT;
    for (uint32_t t = offsets[g]; t < offsets[g + 1] && coeffs; t++)
        if (!has_features || has_features[members[t]]) return members[t];
    return members[offsets[g]];
}

extern "C" int rph_group_max_dist_host(const uint8_t *hashes32, const float *coeffs, const uint8_t *has_features, uint64_t n, const uint32_t *members,
                                       const uint32_t *offsets, uint32_t n_groups, const uint32_t *pivots, uint32_t *max_dist_out, uint32_t *member_dist_out)
{
    return rph_guarded("rph_group_max_dist_host", [&]() -> int {
        RPH_TRY(rph_host_group_lists_check("rph_group_max_dist_host", hashes32, n, members, offsets, n_groups, pivots, max_dist_out));
        uint8_t rows[8 * 32];
        for (uint32_t g = 0; g < n_groups; g++) {
            const uint32_t p = pivots ? pivots[g] : rph_host_default_pivot(members, offsets, g, coeffs, has_features);
            uint32_t n_rows = 0;
            if (p != RPH_NO_PIVOT && coeffs && (!has_features || has_features[p])) {
                rph_pdq_dihedral_one(coeffs + (size_t)p * 256, rows);
                n_rows = 8;
            } else if (p != RPH_NO_PIVOT) {
                std::memcpy(rows, hashes32 + (size_t)p * 32, 32);
                n_rows = 1;
            }
            uint32_t most = 0;
            for (uint32_t t = offsets[g]; t < offsets[g + 1]; t++) {
                uint32_t d = n_rows ? 256 : 0;
                for (uint32_t k = 0; k < n_rows; k++) d = std::min(d, rph_hamming_distance256(rows + k * 32, hashes32 + (size_t)members[t] * 32));
                if (member_dist_out) member_dist_out[t] = d;
                most = std::max(most, d);
            }
            max_dist_out[g] = most;
        }
        return RPH_OK;
    });
}

// ---------------------------------------------------------------------------------------------
// The nearest files of a query (include/rupphash.h): the rule on the host
// ---------------------------------------------------------------------------------------------
int rph_nearest_check(const char *who, const void *rows, uint32_t n_variants, uint64_t n_lib, const void *hashes_q, uint64_t n_q, uint32_t k, const void *out)
{
    const auto refuse = [&](const char *what) {
        rph_set_error("%s: %s", who, what);
        return RPH_ERR_INVALID_ARG;
    };
    if (k < 1 || k > RPH_NEAREST_MAX_K) return refuse("k is not in 1 .. RPH_NEAREST_MAX_K");
    if (n_variants != 1 && n_variants != 8) return refuse("n_variants is neither 1 nor 8");
    if (n_lib >= RPH_NO_FILE) return refuse("at most 2^32 - 2 files");
    if (n_q > 0xFFFFFFFFull) return refuse("at most 2^32 - 1 queries");
    if ((!rows && n_lib) || ((!hashes_q || !out) && n_q)) return refuse("null argument");
    return RPH_OK;
}

extern "C" int rph_hamming_nearest_host(const uint8_t *rows, uint32_t n_variants, const uint8_t *has_features, uint64_t n_lib, const uint8_t *hashes32_q,
                                        const uint32_t *skip, uint64_t n_q, uint32_t k, uint32_t max_dist, rph_edge *out, uint32_t *counts_out)
{
    return rph_guarded("rph_hamming_nearest_host", [&]() -> int {
        RPH_TRY(rph_nearest_check("rph_hamming_nearest_host", rows, n_variants, n_lib, hashes32_q, n_q, k, out));
        // one query per task; its list is the k smallest keys (dist, file, variant) seen so far, ascending
        parallel_for(0, n_q, rph_host_threads(), [&](size_t q) {
            uint64_t best[RPH_NEAREST_MAX_K];
            uint32_t filled = 0;
            const uint8_t *h = hashes32_q + q * 32;
            const uint32_t skipped = skip ? skip[q] : RPH_NO_FILE;
            for (uint64_t i = 0; i < n_lib; i++) {
                if (i == skipped) continue;
                const uint32_t owned = (has_features && !has_features[i]) ? 1 : n_variants;
                uint32_t d = 257, variant = 0;
                for (uint32_t v = 0; v < owned; v++) {
                    const uint32_t dv = rph_hamming_distance256(rows + (i * n_variants + v) * 32, h);
                    if (dv < d) d = dv, variant = v;
                }
                if (d > max_dist) continue;
                const uint64_t key = (uint64_t)d << 40 | i << 3 | variant;
                if (filled == k && key > best[k - 1]) continue;
                uint32_t at = filled < k ? filled++ : k - 1;
                for (; at > 0 && best[at - 1] > key; at--) best[at] = best[at - 1];
                best[at] = key;
            }
            for (uint32_t r = 0; r < k; r++) {
                rph_edge e = {RPH_NO_FILE, (uint32_t)q, 0xFFFF, 0};
                if (r < filled) e = {(uint32_t)(best[r] >> 3), (uint32_t)q, (uint16_t)(best[r] >> 40), (uint16_t)((best[r] & 7) << RPH_EDGE_VARIANT_SHIFT)};
                out[q * k + r] = e;
            }
            if (counts_out) counts_out[q] = filled;
        });
        return RPH_OK;
    });
}
