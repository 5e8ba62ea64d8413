"""The sharded opening (kzg_open_shard_begin / _finish, include/kzg_mi355x.h) restated in plain Python: ints modulo r
and nothing else (a plain module, no fixtures, no import of the package or of the oracle).  The CPU tests pin this
restatement to the oracle's unsharded opening; the GPU tests compare every rank's device results with it.

Rank g holds the coefficients [lo_g, hi_g) of every polynomial, lo_g = b_g, hi_g = b_(g+1).  With the combination
c = sum_i xi^(i+1) p_i (kzg.py:148-150) and its suffix values S_j = c_j + z S_(j+1) (S_0 = c(z), S_j = quotient
coefficient j-1, kzg.py:153-154) the opening proof is (sum_(j >= 1) S_j tau^(j-1)) G1: a sum over j that splits by
rank without any division by tau - z, so it also holds at z = tau."""
from collections import namedtuple

ShardedOpen = namedtuple("ShardedOpen", "c S H carry ev scalar")


def restate_sharded_open(polys, xi, z, bounds, tau, r):
    """polys: coefficient lists (ints), bounds: 0 = b_0 < b_1 < ... < b_G with b_G >= the longest length.
    -> ShardedOpen(c, S, H, carry, ev, scalar):
      c       the combination, zero-padded to b_G coefficients
      S       S_0 .. S_(b_G) (the last one is 0)
      H[g]    sum_j c_(lo_g + j) z^j: what begin returns on rank g
      carry[g]  sum_(g' > g) H_g' z^(lo_g' - hi_g): what the ranks' exchange hands rank g
      ev[g]   what finish leaves in eval_out: S_0 on the first rank, S_(lo_g) on the others
      scalar[g]  trapdoor scalar of rank g's partial point: sum_j S_j tau^(j-1) over j = 1 .. hi_0 - 1 on the first
                 rank and j = lo_g .. hi_g - 1 on the others"""
    bounds = list(bounds)
    G, N = len(bounds) - 1, bounds[-1]
    assert G >= 1 and bounds[0] == 0 and all(a < b for a, b in zip(bounds, bounds[1:]))
    assert all(len(p) <= N for p in polys)
    xi, z, tau = xi % r, z % r, tau % r
    c = [0] * N
    xp = 1
    for p in polys:
        xp = xp * xi % r
        for j, a in enumerate(p):
            c[j] = (c[j] + xp * a) % r
    S = [0] * (N + 1)
    for j in range(N - 1, -1, -1):
        S[j] = (c[j] + z * S[j + 1]) % r
    H = []
    for lo, hi in zip(bounds, bounds[1:]):
        h = 0
        for j in range(hi - 1, lo - 1, -1):
            h = (h * z + c[j]) % r
        H.append(h)
    carry = [sum(H[g2] * pow(z, bounds[g2] - bounds[g + 1], r) for g2 in range(g + 1, G)) % r for g in range(G)]
    ev = [S[bounds[g]] for g in range(G)]
    scalar = []
    for g in range(G):
        first = max(bounds[g], 1)
        acc, tp = 0, pow(tau, first - 1, r)
        for j in range(first, bounds[g + 1]):
            acc = (acc + S[j] * tp) % r
            tp = tp * tau % r
        scalar.append(acc)
    return ShardedOpen(c, S, H, carry, ev, scalar)


def derivative_at(c, x, r):
    """value at x of the formal derivative of the coefficient list c"""
    return sum(j * a % r * pow(x, j - 1, r) for j, a in enumerate(c) if j) % r
