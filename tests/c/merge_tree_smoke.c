/* A plain C99 consumer of the merge-tree calls that need no device (include/rupphash.h, "Merge tree"): the tree of a hand-made edge
 * list, cut at two similarities.  Built and run by tests/test_merge_tree_cpu.py. */
#include <stdio.h>

#include "rupphash.h"

int main(void)
{
    /* 2-3, 1-2 and 0-1 all at level 9: file 3 ends in 0, whatever joined it first; 4-5 at level 2; 5-0 at level 20 */
    const rph_edge edges[5] = {{2, 3, 9, 0}, {1, 2, 9, 0}, {0, 1, 9, 0}, {4, 5, 2, 0}, {5, 0, 20, 0}};
    uint32_t into[6], labels[6], members[6], offsets[5], n_groups = 0;
    uint8_t level[6];
    uint64_t edges_at[21], groups[21], grouped[21];
    int x;
    if (rph_merge_tree_from_edges_host(edges, 5, 6, 20, into, level, edges_at) != RPH_OK) return 1;
    for (x = 0; x < 6; x++) printf("file %d: into %u at level %u\n", x, into[x], level[x]);
    if (into[3] != 0 || level[3] != 9 || level[0] != RPH_TREE_NEVER || into[4] != 0 || level[4] != 20 || into[5] != 4 || level[5] != 2) return 2;
    if (edges_at[9] != 3 || edges_at[2] != 1 || edges_at[20] != 1 || edges_at[0] != 0) return 3;
    if (rph_merge_tree_labels(into, level, 6, 9, labels) != RPH_OK || labels[3] != 0 || labels[5] != 4) return 4;
    if (rph_merge_tree_groups(into, level, 6, 9, members, offsets, &n_groups) != RPH_OK || n_groups != 2 || offsets[1] != 4 || offsets[2] != 6) return 5;
    if (rph_merge_tree_groups(into, level, 6, 20, members, offsets, &n_groups) != RPH_OK || n_groups != 1 || offsets[1] != 6) return 6;
    if (rph_merge_tree_profile(into, level, 6, 20, groups, grouped) != RPH_OK || groups[1] != 0 || groups[2] != 1 || groups[9] != 2 || groups[20] != 1 ||
        grouped[2] != 2 || grouped[9] != 6)
        return 7;
    into[3] = 5; /* malformed: refused, nothing written */
    labels[0] = 77;
    if (rph_merge_tree_labels(into, level, 6, 9, labels) != RPH_ERR_INVALID_ARG || labels[0] != 77) return 8;
    printf("merge tree ok\n");
    return 0;
}
