// host_merge_tree.cpp -- the merge tree on the host (include/rupphash.h, "Merge tree"): the rule restated without a device
// (rph_merge_tree_host, rph_merge_tree_from_edges_host) and the calls that cut a tree, which are host work in every form: one pass over
// n records of five bytes.
//   grouping rule               scanner.rs:1640-1817
//   variants, low confidence    scanner.rs:1692-1701, 1721
#include <algorithm>
#include <cstring>
#include <vector>

#include "rph_internal.h"

namespace {
int fail(const char *who, const char *what)
{
    rph_set_error("%s: %s", who, what);
    return RPH_ERR_INVALID_ARG;
}

uint32_t find(std::vector<uint32_t> &parent, uint32_t x)
{
    while (parent[x] != x) {
        parent[x] = parent[parent[x]];
        x = parent[x];
    }
    return x;
}

// RPH_ERR_INVALID_ARG unless (into, level) can be the tree of some edge list: into[x] <= x; into[x] == x exactly when level[x] is NEVER;
// the level rises along every chain.  One pass, nothing written.
int check_tree(const char *who, const uint32_t *into, const uint8_t *level, uint64_t n)
{
    if ((!into || !level) && n) return fail(who, "null argument");
    if (n > 0x7FFFFFFFull) return fail(who, "at most 2^31 - 1 files");
    for (uint64_t x = 0; x < n; x++) {
        const uint32_t p = into[x];
        if (p > x) return fail(who, "malformed tree: into[x] lies above x");
        if ((p == x) != (level[x] == RPH_TREE_NEVER)) return fail(who, "malformed tree: into[x] == x and level[x] != RPH_TREE_NEVER, or the reverse");
        if (p != x && level[p] <= level[x]) return fail(who, "malformed tree: the level does not rise along a chain");
    }
    return RPH_OK;
}

// label_s of a checked tree: into[x] < x, so the label of into[x] is there when x needs it
void cut_labels(const uint32_t *into, const uint8_t *level, uint64_t n, uint32_t s, uint32_t *labels)
{
    for (uint64_t x = 0; x < n; x++) labels[x] = level[x] != RPH_TREE_NEVER && level[x] <= s ? labels[into[x]] : (uint32_t)x;
}

int check_top_pdq(const char *who, uint32_t top)
{
    if (top <= RPH_MAX_SIMILARITY_256) return RPH_OK;
    rph_set_error("%s: Similarity distances above %u require R=4 bit-flip checks, which are not implemented.", who, RPH_MAX_SIMILARITY_256);
    return RPH_ERR_INVALID_ARG;
}
}  // namespace

// Kruskal by level: the edges into level buckets (counting sort), then per level the union-find that hooks the larger root under the
// smaller.  A root that is hooked gets its level at once and its `into` behind the level's last union, when the roots are final.
void rph_host_merge_tree(const rph_edge *edges, uint64_t n_edges, uint64_t n, uint32_t top, uint32_t *into, uint8_t *level)
{
    std::vector<uint64_t> start(top + 2, 0);
    for (uint64_t e = 0; e < n_edges; e++) start[edges[e].d + 1]++;
    for (uint32_t t = 0; t <= top; t++) start[t + 1] += start[t];
    std::vector<uint32_t> a(n_edges), b(n_edges), parent(n), hooked;
    {
        std::vector<uint64_t> at(start.begin(), start.end() - 1);
        for (uint64_t e = 0; e < n_edges; e++) {
            const uint64_t k = at[edges[e].d]++;
            a[k] = edges[e].i, b[k] = edges[e].j;
        }
    }
    for (uint64_t x = 0; x < n; x++) parent[x] = into[x] = (uint32_t)x, level[x] = RPH_TREE_NEVER;
    for (uint32_t t = 0; t <= top; t++) {
        hooked.clear();
        for (uint64_t k = start[t]; k < start[t + 1]; k++) {
            const uint32_t ra = find(parent, a[k]), rb = find(parent, b[k]);
            if (ra == rb) continue;
            const uint32_t hi = std::max(ra, rb);
            parent[hi] = std::min(ra, rb);
            level[hi] = (uint8_t)t;
            hooked.push_back(hi);
        }
        for (uint32_t x : hooked) into[x] = find(parent, x);
    }
}

// The cut of rph_merge_tree_truncate on a checked tree: each output is written from the input at the same index, so the outputs may be the inputs
void rph_host_merge_tree_cut(const uint32_t *into, const uint8_t *level, uint64_t n, uint32_t t, uint32_t *into_out, uint8_t *level_out)
{
    for (uint64_t x = 0; x < n; x++) {
        const bool stays = level[x] <= t;  // (RPH_TREE_NEVER is above every t)
        into_out[x] = stays ? into[x] : (uint32_t)x;
        level_out[x] = stays ? level[x] : (uint8_t)RPH_TREE_NEVER;
    }
}

extern "C" {

int rph_merge_tree_from_edges_host(const rph_edge *edges, uint64_t n_edges, uint64_t n, uint32_t top, uint32_t *into, uint8_t *level, uint64_t *edges_at)
{
    return rph_guarded("rph_merge_tree_from_edges_host", [&]() -> int {
        const char *who = "rph_merge_tree_from_edges_host";
        if ((!edges && n_edges) || ((!into || !level) && n) || !edges_at) return fail(who, "null argument");
        if (n > 0x7FFFFFFFull) return fail(who, "at most 2^31 - 1 files");
        if (top >= RPH_TREE_NEVER) return fail(who, "top at most 254: level 255 is RPH_TREE_NEVER");
        for (uint64_t e = 0; e < n_edges; e++)
            if (edges[e].i >= n || edges[e].j >= n || edges[e].d > top) return fail(who, "an edge names a file outside n or a distance above top");
        std::fill(edges_at, edges_at + top + 1, 0);
        for (uint64_t e = 0; e < n_edges; e++) edges_at[edges[e].d]++;
        rph_host_merge_tree(edges, n_edges, n, top, into, level);
        return RPH_OK;
    });
}

// Brute force: file i's rows against every hash j > i, one task per i, every passing (row, j) an edge as the variant sweep reports it.
int rph_merge_tree_host(const uint8_t *hashes32, const float *coeffs, const uint8_t *has_features, const int32_t *quality, uint64_t n, uint32_t top, uint32_t *into,
                        uint8_t *level, uint64_t *edges_at)
{
    return rph_guarded("rph_merge_tree_host", [&]() -> int {
        const char *who = "rph_merge_tree_host";
        if ((!hashes32 && n) || ((!into || !level) && n) || !edges_at) return fail(who, "null argument");
        if (n > 0x7FFFFFFFull) return fail(who, "at most 2^31 - 1 files");
        RPH_TRY(check_top_pdq(who, top));
        const unsigned threads = rph_host_threads();
        std::vector<std::vector<rph_edge>> found(n);
        parallel_for(0, n, threads, [&](size_t i) {
            uint8_t rows[8 * 32];
            uint32_t n_rows = 1;
            if (coeffs && (!has_features || has_features[i])) {
                rph_pdq_dihedral_one(coeffs + i * 256, rows);
                n_rows = 8;
            } else {
                std::memcpy(rows, hashes32 + i * 32, 32);
            }
            const bool low_i = quality && rph_is_low_pdq_quality(quality[i]);
            for (uint64_t j = i + 1; j < n; j++) {
                const uint32_t limit = low_i || (quality && rph_is_low_pdq_quality(quality[j])) ? 0 : top;
                for (uint32_t v = 0; v < n_rows; v++) {
                    const uint32_t d = rph_hamming_distance256(rows + v * 32, hashes32 + j * 32);
                    if (d <= limit) found[i].push_back({(uint32_t)i, (uint32_t)j, (uint16_t)d, (uint16_t)(v << RPH_EDGE_VARIANT_SHIFT)});
                }
            }
        });
        std::vector<rph_edge> edges;
        for (auto &f : found) edges.insert(edges.end(), f.begin(), f.end());
        std::fill(edges_at, edges_at + top + 1, 0);
        for (const rph_edge &e : edges) edges_at[e.d]++;
        rph_host_merge_tree(edges.data(), edges.size(), n, top, into, level);
        return RPH_OK;
    });
}

int rph_merge_tree_labels(const uint32_t *into, const uint8_t *level, uint64_t n, uint32_t s, uint32_t *labels_out)
{
    return rph_guarded("rph_merge_tree_labels", [&]() -> int {
        if (!labels_out && n) return fail("rph_merge_tree_labels", "null argument");
        RPH_TRY(check_tree("rph_merge_tree_labels", into, level, n));
        cut_labels(into, level, n, s, labels_out);
        return RPH_OK;
    });
}

// level[x] is the smallest s at which x stops being its own label, whatever `top` the tree was built for: the tree for t keeps the
// records with level <= t and turns the others into roots.  Each output is written from the input at the same index, so the outputs may
// be the inputs.
int rph_merge_tree_truncate(const uint32_t *into, const uint8_t *level, const uint64_t *edges_at, uint64_t n, uint32_t top, uint32_t t, uint32_t *into_out,
                            uint8_t *level_out, uint64_t *edges_at_out)
{
    return rph_guarded("rph_merge_tree_truncate", [&]() -> int {
        const char *who = "rph_merge_tree_truncate";
        if (!edges_at || !edges_at_out || ((!into_out || !level_out) && n)) return fail(who, "null argument");
        if (top >= RPH_TREE_NEVER) return fail(who, "top at most 254: level 255 is RPH_TREE_NEVER");
        if (t > top) return fail(who, "t above the top the tree was built for");
        RPH_TRY(check_tree(who, into, level, n));
        rph_host_merge_tree_cut(into, level, n, t, into_out, level_out);
        if (edges_at_out != edges_at) std::memmove(edges_at_out, edges_at, (size_t)(t + 1) * 8);
        return RPH_OK;
    });
}

int rph_merge_tree_groups(const uint32_t *into, const uint8_t *level, uint64_t n, uint32_t s, uint32_t *members, uint32_t *offsets, uint32_t *n_groups_out)
{
    return rph_guarded("rph_merge_tree_groups", [&]() -> int {
        if (!members || !offsets || !n_groups_out) return fail("rph_merge_tree_groups", "null argument");
        RPH_TRY(check_tree("rph_merge_tree_groups", into, level, n));
        // a label is its component's first member, so the groups in label order are the groups by first member; members ascend
        std::vector<uint32_t> labels(n), count(n, 0), at(n, 0);
        cut_labels(into, level, n, s, labels.data());
        for (uint64_t x = 0; x < n; x++) count[labels[x]]++;
        uint32_t ng = 0, total = 0;
        offsets[0] = 0;
        for (uint64_t x = 0; x < n; x++)
            if (count[x] > 1) {
                at[x] = total;
                total += count[x];
                offsets[++ng] = total;
            }
        for (uint64_t x = 0; x < n; x++)
            if (count[labels[x]] > 1) members[at[labels[x]]++] = (uint32_t)x;
        *n_groups_out = ng;
        return RPH_OK;
    });
}

// No pass per level.  The roots at s are the x with level[x] > s, and such a root is alone at s iff no y with into[y] == x has joined by
// then: first_join[x] = min level[y] over those y.  So x is a component of more than one member for first_join[x] <= s < level[x], and a
// file is in such a component from s = min(first_join[x], level[x]) on: two histograms and their running sums.
int rph_merge_tree_profile(const uint32_t *into, const uint8_t *level, uint64_t n, uint32_t top, uint64_t *n_groups_out, uint64_t *grouped_files_out)
{
    return rph_guarded("rph_merge_tree_profile", [&]() -> int {
        if (!n_groups_out || !grouped_files_out) return fail("rph_merge_tree_profile", "null argument");
        if (top >= RPH_TREE_NEVER) return fail("rph_merge_tree_profile", "top at most 254: level 255 is RPH_TREE_NEVER");
        RPH_TRY(check_tree("rph_merge_tree_profile", into, level, n));
        std::vector<uint8_t> first_join(n, RPH_TREE_NEVER);
        for (uint64_t y = 0; y < n; y++)
            if (level[y] != RPH_TREE_NEVER) first_join[into[y]] = std::min(first_join[into[y]], level[y]);
        uint64_t becomes_group[257] = {0}, absorbed[257] = {0}, joins[257] = {0};
        for (uint64_t x = 0; x < n; x++) {
            if (first_join[x] != RPH_TREE_NEVER) becomes_group[first_join[x]]++, absorbed[level[x]]++;  // (absorbed[255]: never)
            joins[std::min(first_join[x], level[x])]++;
        }
        uint64_t groups = 0, files = 0;
        for (uint32_t s = 0; s <= top; s++) {
            groups += becomes_group[s] - absorbed[s], files += joins[s];
            n_groups_out[s] = groups;
            grouped_files_out[s] = files;
        }
        return RPH_OK;
    });
}

}  // extern "C"
