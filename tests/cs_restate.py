"""A plain NumPy/Python restatement of the local credible sets, written from the definitions and not from the
kernels: the history's words, the counts, the friends of a lead, the candidate sets with their PEP, the walk over the candidates,
and the text of the .cs table.  Everything is integer; no test of its own."""
import math

import numpy as np

NONE = 0xFFFFFFFF


class History:
    """C chains x T planned records over M markers.  Record q = t C + r (t adds so far, chain r); marker j's bit q lies in
    words[q // 64, j] at bit q % 64; NW = ceil(C T / 64) words per marker; every bit at or above the records added is 0."""

    def __init__(self, C, T, M):
        self.C, self.T, self.M, self.t = C, T, M, 0
        self.words = np.zeros(((C * T + 63) // 64, M), dtype=np.uint64)

    def add(self, flags):
        """one record of every chain: flags (C, M), non-zero = in the model"""
        flags = np.asarray(flags).reshape(self.C, self.M) != 0
        assert self.t < self.T
        for r in range(self.C):
            q = self.t * self.C + r
            self.words[q // 64, flags[r]] |= np.uint64(1 << (q % 64))
        self.t += 1

    @property
    def nrec(self):
        return self.t * self.C

    def counts(self):
        return popcount(self.words).sum(axis=0).astype(np.uint32)


def popcount(a):
    """per element of a uint64 array"""
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return np.unpackbits(a.view(np.uint8).reshape(a.shape + (8,)), axis=-1).sum(axis=-1)


def friends(v, M, W, fwd, bwd):
    """the friends of lead v on masks (M, wpr) uint64 in hgibbs_ld_mask's layout: v + d iff bit d - 1 of v's forward row, v - d iff
    bit d - 1 of its backward row; nothing else, and no marker that does not exist"""
    out = []
    for d in range(1, W + 1):
        w, b = (d - 1) // 64, (d - 1) % 64
        if v + d < M and (int(fwd[v, w]) >> b) & 1:
            out.append(v + d)
        if v - d >= 0 and (int(bwd[v, w]) >> b) & 1:
            out.append(v - d)
    return out


def candidate(v, cnt, words, M, W, fwd, bwd, need, max_size, notes=None):
    """The candidate set of lead v: (status, size, sum, pep, members padded to max_size with NONE).  notes, a dict, collects what the
    tests' conditions ask about: 'tie' (a pick decided by the index among equal counts) and 'zero' (a friend with cnt 0 was left
    while the set still needed more)."""
    assert need >= 1 and 1 <= max_size <= 256
    members, total = [v], int(cnt[v])
    fr = friends(v, M, W, fwd, bwd)
    status = 0
    while total < need:
        if len(members) == max_size:
            status = 2
            break
        rest = [q for q in fr if q not in members and cnt[q] > 0]
        if notes is not None and any(cnt[q] == 0 for q in fr):
            notes["zero"] = True
        if not rest:
            status = 1
            break
        top = max(int(cnt[q]) for q in rest)
        best = sorted(q for q in rest if cnt[q] == top)
        if notes is not None and len(best) > 1:
            notes["tie"] = True
        members.append(best[0])
        total += top
    if status:
        return status, 0, total, 0, [NONE] * max_size
    union = np.zeros(words.shape[0], dtype=np.uint64)
    for q in members:
        union |= words[:, q]
    return 0, len(members), total, int(popcount(union).sum()), members + [NONE] * (max_size - len(members))


def candidates(leads, cnt, words, M, W, fwd, bwd, need, max_size, notes=None):
    """status, size (n,) uint32, sum (n,) uint64, pep (n,) uint32, members (n, max_size) uint32 of the leads in their order"""
    res = [candidate(int(v), cnt, words, M, W, fwd, bwd, need, max_size, notes) for v in leads]
    n = len(res)
    return (np.array([r[0] for r in res], dtype=np.uint32), np.array([r[1] for r in res], dtype=np.uint32), np.array([r[2] for r in res], dtype=np.uint64),
            np.array([r[3] for r in res], dtype=np.uint32), np.array([r[4] for r in res], dtype=np.uint32).reshape(n, max_size))


def walk(leads, lead_cnt, status, size, pep, members, min_pep):
    """The selection: candidates by descending count of the lead, ties by ascending lead index; one is accepted iff its status is 0,
    its pep >= min_pep and none of its members belongs to an accepted set.  Returns the accepted positions in the order taken."""
    order = sorted(range(len(leads)), key=lambda i: (-int(lead_cnt[i]), int(leads[i])))
    owned, taken = set(), []
    for i in order:
        if status[i] != 0 or pep[i] < min_pep:
            continue
        mem = [int(q) for q in members[i][:int(size[i])]]
        if any(q in owned for q in mem):
            continue
        owned.update(mem)
        taken.append(i)
    return taken


def ceil_count(x, nrec):
    """x of nrec records as a count: (uint32) ceil(x * (double) nrec), at least 1"""
    return max(1, int(math.ceil(x * float(nrec))))


def lead_list(cnt, lead, nrec):
    """the leads of the command line: the markers with cnt >= ceil(lead nrec), ascending"""
    return np.flatnonzero(cnt >= ceil_count(lead, nrec)).astype(np.uint32)


def table_text(ids, chrs, bps, nrec, cnt, leads, size, total, pep, members, taken):
    """the .cs table of the accepted sets in the order taken"""
    out = ["CS\tLEAD\tCHR\tBP_FIRST\tBP_LAST\tSIZE\tNREC\tPIP_LEAD\tPIP_SUM\tPEP\tSNPS\tPIPS"]
    n = float(nrec)
    for k, i in enumerate(taken):
        v = int(leads[i])
        mem = [int(q) for q in members[i][:int(size[i])]]
        bp = [int(bps[q]) for q in mem]
        out.append("\t".join([str(k + 1), ids[v], str(chrs[v]), str(min(bp)), str(max(bp)), str(int(size[i])), str(nrec), "%.9g" % (float(cnt[v]) / n),
                              "%.9g" % (float(total[i]) / n), "%.9g" % (float(pep[i]) / n), ",".join(ids[q] for q in mem),
                              ",".join("%.9g" % (float(cnt[q]) / n) for q in mem)]))
    return "\n".join(out) + "\n"


def sets_table(ids, chrs, bps, nrec, cnt, words, M, W, fwd, bwd, alpha=0.9, pep=0.7, lead=0.01, max_size=64):
    """steps 2, 4 and 5 of the command line on given counts, words and masks, then the table: (text, leads, results, taken)"""
    leads = lead_list(cnt, lead, nrec)
    res = candidates(leads, cnt, words, M, W, fwd, bwd, ceil_count(alpha, nrec), max_size)
    status, size, total, p, members = res
    taken = walk(leads, cnt[leads], status, size, p, members, ceil_count(pep, nrec))
    return table_text(ids, chrs, bps, nrec, cnt, leads, size, total, p, members, taken), leads, res, taken
