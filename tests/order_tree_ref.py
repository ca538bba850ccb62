"""numpy restatement of mmseq_order_tree's index rule (include/mmseq.h, csrc/order_tree_plan.h):
the prefix tree over all N! orders, its node counts, the child index and the unranked table.

A node of level t (t picks made) with index i has the children i * (N - t) + r, r = 0 .. N-t-1, the
child r picking the r-th still-unpointed step in ASCENDING order; a node of level N - 1 is its
order's rank among the permutations of 0 .. N-1 in lexicographic order. `rule` names the rank rule
so that the tests can show that the wrong ones do not give that table.
"""
import math

import numpy as np


def level_width(N, t):
    """Nodes of level t per story: N! / (N - t)!."""
    return math.factorial(N) // math.factorial(N - t)


def node_steps(N):
    """Prefixes stepped per story: levels 0 .. N-2."""
    return sum(level_width(N, t) for t in range(N - 1))


def flat_steps(N):
    """Steps of the flat scorer over all N! orders."""
    return math.factorial(N) * (N - 1)


def child_index(N, t, i, r):
    return i * (N - t) + r


def pick(N, prefix, r, rule="ascending"):
    """The step the r-th child of a node with picks `prefix` takes."""
    free = [j for j in range(N) if j not in prefix]
    if rule == "ascending":
        return free[r]
    if rule == "descending":
        return free[::-1][r]
    if rule == "all_steps":  # r counted over all steps instead of the unpointed ones
        return r
    raise ValueError(rule)


def unrank_table(N, rule="ascending"):
    """orders int64 [N!][N] by walking the tree level by level with `child_index` and `pick`; the
    last position takes the one step left."""
    nodes = {0: ()}
    for t in range(N - 1):
        nxt = {}
        for i, prefix in nodes.items():
            for r in range(N - t):
                nxt[child_index(N, t, i, r)] = prefix + (pick(N, prefix, r, rule),)
        nodes = nxt
    out = np.zeros((math.factorial(N), N), np.int64)
    assert sorted(nodes) == list(range(len(out)))
    for i, prefix in nodes.items():
        rest = [j for j in range(N) if j not in prefix]
        out[i] = list(prefix) + rest[:1] if N > 1 else [0]
    return out


def unrank(N, k):
    """The k-th permutation from the digits of k in the factorial number system (what the unrank
    kernel computes), without the tree."""
    free, out, rem = list(range(N)), [], int(k)
    for p in range(N):
        f = math.factorial(N - 1 - p)
        out.append(free.pop(rem // f))
        rem %= f
    return out
