"""numpy restatement of the balanced breaker (include/ctd_hip.h, "shaped fit, balanced lines") on top of `fit_ref`: the row of
the shaped fit gives the candidate, the line count and the slots' widths; the whole backward table g(k, s) over EVERY start
0 .. G follows from the rule's statement, one numpy pass per line length (all lines of d glyphs at once), and a forward pass
takes the largest end that attains it.  Nothing of the kernel's is here: no band between a backward and a forward greedy, no
binary search, no compact table (csrc/kernels_fit.hip).  tests/test_balance_ref.py holds it against an enumeration of every
break vector; tests/test_gpu_balance.py compares the kernel with `balance_row` field by field."""
import numpy as np

import balloon_ref as BR
import fit_ref as FR

INF = 1 << 62
BAL_FIELDS = ("balanced", "cost")


def boundaries(G, breaks=None):
    """ok[e] for e in 0 .. G: a line may end in front of glyph e (e = G, no break table, or the byte of glyph e - 1)."""
    ok = np.ones((G + 1,), bool)
    if breaks is not None:
        ok[1:] = np.asarray(breaks).astype(bool)[:G]
    ok[0], ok[G] = False, True
    return ok


def table(cum, widths, breaks=None):
    """g[k, s] for k in 0 .. n and s in 0 .. G: the least cost of lines k .. n - 1 where line k starts at glyph s, INF where
    they cannot hold glyphs s .. G - 1.  g[n, G] = 0."""
    cum = np.asarray(cum, np.int64)
    G, n = len(cum) - 1, len(widths)
    ok = boundaries(G, breaks)
    g = np.full((n + 1, G + 1), INF, np.int64)
    g[n, G] = 0
    for k in range(n - 1, -1, -1):
        w = int(widths[k])
        for d in range(1, G + 1):                           # every line of d glyphs: s .. s + d - 1
            s = np.arange(G + 1 - d)
            e = s + d
            ln = cum[e] - cum[s]
            fits = ln <= w
            if not fits.any():
                break                                       # the advances do not decrease: no longer line fits either
            good = fits & ok[e] & (g[k + 1, e] < INF)
            cost = np.where(good, (w - ln) ** 2 + np.where(good, g[k + 1, e], 0), INF)
            g[k, s] = np.minimum(g[k, s], cost)
    return g


def balanced(cum, widths, breaks=None):
    """([(start, end)] of len(widths) lines, cost): the admissible vector of least cost, among equals the lexicographically
    largest; None where there is none."""
    cum = np.asarray(cum, np.int64)
    G, n = len(cum) - 1, len(widths)
    if G < 1 or n < 1:
        return None
    ok = boundaries(G, breaks)
    g = table(cum, widths, breaks)
    if g[0, 0] >= INF:
        return None
    lines, s = [], 0
    for k in range(n):
        e = np.arange(s + 1, G + 1)
        ln = cum[e] - cum[s]
        good = (ln <= widths[k]) & ok[e] & (g[k + 1, e] < INF)
        hit = e[good][(int(widths[k]) - ln[good]) ** 2 + g[k + 1, e[good]] == g[k, s]]
        lines.append((s, int(hit.max())))
        s = lines[-1][1]
    return lines, int(g[0, 0])


def cost_of(cum, widths, lines):
    return sum((int(w) - int(cum[e] - cum[s])) ** 2 for w, (s, e) in zip(widths, lines))


def _zero_bal():
    return dict(balanced=0, cost=0)


def rebalance(row, cums, breaks=None):
    """(row, balance row) from a `fit_ref.fit_row` row: `start` and `length` of its line records from `balanced` where an
    admissible vector exists, and {balanced, cost}; the row as it is and all 0 in any status but OK."""
    if row["status"] != FR.OK:
        return row, _zero_bal()
    n, cum = row["n_lines"], [int(v) for v in cums[row["cand"]]]
    recs = row["lines"][:n]
    got = balanced(cum, [r[3] for r in recs], breaks)
    if got is None:
        return row, dict(balanced=0, cost=sum((r[3] - r[4]) ** 2 for r in recs))
    out = dict(row)
    out["lines"] = [[s, r[1], r[2], r[3], cum[e] - cum[s]] for r, (s, e) in zip(recs, got[0])] + row["lines"][n:]
    return out, dict(balanced=1, cost=got[1])


def balance_row(region, win, anchor, cums, lines, gaps, breaks=None, inset=2, balloon_status=BR.OK, max_words=BR.MAX_WORDS):
    """(row, balance row) of one block: `rebalance` of its `fit_ref.fit_row`."""
    return rebalance(FR.fit_row(region, win, anchor, cums, lines, gaps, breaks=breaks, inset=inset, balloon_status=balloon_status,
                                max_words=max_words), cums, breaks)


def bal_dict(rec):
    """A record of the kernel's balance table as the dict `balance_row` returns (the padding must be 0)."""
    assert int(rec["pad_"]) == 0
    return {k: int(rec[k]) for k in BAL_FIELDS}


def word_breaks(G, rng):
    """Words of 2 .. 7 glyphs, each followed by one breakable glyph."""
    br, i = np.zeros((G,), bool), 0
    while i < G:
        i += int(rng.integers(2, 8))
        if i < G:
            br[i] = True
            i += 1
    return br
