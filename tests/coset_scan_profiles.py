"""The division by X^l - a behind kzg_open_coset (csrc/poly.hip: coset_tile_kernel, coset_fill_kernel, coset_scan_level
and open_coset_quotient_t), restated on Python integers, and the shapes tests/test_open_coset_scan_gpu.py runs.  Pure
Python: no GPU, no library.

    coset_divide    (quotient, remainder) by the plain suffix recursion S_t = c_t + a S_(t+l): the definition
    blocked_divide  the same through the device's blocked scan -- rows of l coefficients, tiles of CS_R rows, one level
                    per factor of CS_R in the row count, the aggregates of a level scanned by the level above with a^R,
                    every tile filled downwards from the carry of the tile above it.  It exists so that
                    tests/test_coset_scan_profiles_host.py can show that the blocked scan IS the plain one; no GPU
                    expectation is taken from it.
    plan            what one call does: rows, tiles and launches per level, the scratch elements of the aggregates,
                    the ragged tiles, the levels whose last tile reads no carry while the others read one
    cases           the (log_l, n) shapes of the GPU test, labelled; the host test pins what they reach"""
from collections import namedtuple

CS_R = 16                # csrc/poly.hip: constexpr uint32_t CS_R -- rows per tile of the blocked scan
CS_MAX_LOG_L = 12        # csrc/poly.hip: constexpr uint32_t CS_MAX_LOG_L -- kzg_open_coset takes log_l in [0, 12]
BLOCK = 256              # threads per block of both kernels (__launch_bounds__(256), dim3(256))
MAX_N = 1 << 17          # no case is longer


# ---- the definition --------------------------------------------------------------------------------------------------

def coset_divide(coeffs, l, a, r):
    """(quotient, remainder) of p by X^l - a: S_t = c_t + a S_(t+l), q_t = S_(t+l), rho_j = S_j"""
    c = [int(x) % r for x in coeffs]
    S = c + [0] * l
    for t in range(len(c) - 1, -1, -1):
        S[t] = (c[t] + a * S[t + l]) % r
    return [S[t + l] for t in range(max(len(c) - l, 0))], [S[j] for j in range(l)]


# ---- the blocked scan ------------------------------------------------------------------------------------------------

def _tiles(rows):
    return (rows + CS_R - 1) // CS_R


def _tile_aggregates(x, rows, l, a, r):
    """coset_tile_kernel: A[b][j] = sum_(q < R) x[bR + q][j] a^q over the rows that exist"""
    agg = [0] * (_tiles(rows) * l)
    for b in range(_tiles(rows)):
        for j in range(l):
            acc = 0
            for q in range(CS_R - 1, -1, -1):
                row = b * CS_R + q
                if row < rows:
                    acc = (x[row * l + j] + acc * a) % r
            agg[b * l + j] = acc
    return agg


def _fill(x, rows, l, a, upper, upper_rows, r, fault=None):
    """coset_fill_kernel, in place: tile b walks its rows down from the carry upper[b + 1] (zero when there is no level
    above, or no row b + 1 in it)"""
    if fault == "carry" and upper_rows > CS_R:
        upper = None
    for b in range(_tiles(rows)):
        for j in range(l):
            acc = upper[(b + 1) * l + j] if upper is not None and b + 1 < upper_rows else 0
            for q in range(CS_R - 1, -1, -1):
                row = b * CS_R + q
                if row < rows:
                    acc = (x[row * l + j] + acc * a) % r
                    x[row * l + j] = acc


def _scan_level(x, rows, l, a, r, fault=None):
    """coset_scan_level: x (rows x l) becomes its suffix values, in place"""
    tiles = _tiles(rows)
    if tiles == 1:
        _fill(x, rows, l, a, None, 0, r)
        return
    agg = _tile_aggregates(x, rows, l, a, r)
    aR = a
    q = 2 if fault == "power" else 1
    while q < CS_R:                                           # a^R by squarings, as the host code forms it
        aR = aR * aR % r
        q <<= 1
    _scan_level(agg, tiles, l, aR, r, fault)
    _fill(x, rows, l, a, agg, tiles, r, fault)


def blocked_divide(coeffs, l, a, r, fault=None):
    """coset_divide through the blocked scan of open_coset_quotient_t: the coefficients zero-padded to whole rows, the
    scan, the remainder from the first row and the quotient from element l on.
    fault: a deliberately WRONG scan, for the host test's statement of which shapes can tell -- "power": a^R with one
    squaring fewer; "carry": no carry read from a level above of more than CS_R rows."""
    n = len(coeffs)
    if n == 0:
        return [], [0] * l
    rows = (n + l - 1) // l
    x = [int(c) % r for c in coeffs] + [0] * (rows * l - n)
    _scan_level(x, rows, l, a % r, r, fault)
    rho = x[:min(l, n)] + [0] * (l - min(l, n))
    return (x[l:n] if n > l else []), rho


# ---- what one call does ----------------------------------------------------------------------------------------------

Level = namedtuple("Level", "rows tiles ragged carry_absent_last launches")
Launch = namedtuple("Launch", "kernel level threads whole_blocks")
Plan = namedtuple("Plan", "n l rows depth levels agg agg_used launches quotient_len copied")


def plan(n, log_l):
    """One kzg_open_coset call on n > 0 combined coefficients.
    levels[i]: the i-th coset_scan_level call -- its rows, tiles, whether the last tile is ragged (rows no multiple of
    CS_R), whether its fill gives the last tile no carry (b + 1 == upper_rows) while the tiles below it get one (any
    level of two or more tiles; a single tile has no level above), and its launches.
    agg: the elements open_coset_quotient_t reserves for the aggregates; agg_used: those the levels write.
    launches: every launch in stream order, threads = tiles * l each, whole_blocks: a multiple of 256.
    quotient_len = max(n - l, 0); copied = min(l, n) remainder elements come back."""
    assert n > 0 and 0 <= log_l <= CS_MAX_LOG_L
    l = 1 << log_l
    rows = (n + l - 1) >> log_l
    agg = 0
    q = rows
    while q > 1:
        agg += _tiles(q) << log_l
        q = _tiles(q)
    levels, down, up, used = [], [], [], 0
    q, i = rows, 0
    while True:
        tiles = _tiles(q)
        threads = tiles << log_l
        whole = threads % BLOCK == 0
        if tiles == 1:
            mine = [Launch("fill", i, threads, whole)]
            down.append(mine[0])
        else:
            mine = [Launch("tile", i, threads, whole), Launch("fill", i, threads, whole)]
            down.append(mine[0])
            up.append(mine[1])
            used += threads
        levels.append(Level(q, tiles, q % CS_R != 0, tiles >= 2, tuple(mine)))
        if tiles == 1:
            break
        q, i = tiles, i + 1
    return Plan(n, l, rows, len(levels), tuple(levels), agg, used, tuple(down + up[::-1]), max(n - l, 0), min(l, n))


# ---- the shapes of the GPU test --------------------------------------------------------------------------------------

Case = namedtuple("Case", "label log_l n")

ROWS_L1 = (1, 2, 15, 16, 17, 255, 256, 257, 271, 272, 273, 4095, 4096, 4097, 4113, 65537)   # one to five levels
ROWS_BY_LOG_L = {1: (1, 2, 16, 17, 257), 3: (1, 2, 16, 17, 257), 8: (1, 2, 16, 17, 257), 12: (1, 2, 17)}
AROUND_L = (2, 8, 4096)                                       # n < l, n = l and n = l + 1


def cases():
    """[Case]: no (log_l, n) twice, the first label kept"""
    out, seen = [], set()

    def add(label, log_l, n):
        if n >= 1 and (log_l, n) not in seen:
            assert n <= MAX_N
            seen.add((log_l, n))
            out.append(Case(label, log_l, n))

    for rows in ROWS_L1:
        add("l1:rows%d" % rows, 0, rows)
    for log_l, row_counts in sorted(ROWS_BY_LOG_L.items()):
        l = 1 << log_l
        for rows in row_counts:
            add("l%d:rows%d:full" % (l, rows), log_l, rows * l)
            add("l%d:rows%d:short1" % (l, rows), log_l, rows * l - 1)
            add("l%d:rows%d:one" % (l, rows), log_l, (rows - 1) * l + 1)
    for l in AROUND_L:
        log_l = l.bit_length() - 1
        add("l%d:n<l" % l, log_l, l - 1)
        add("l%d:n=l" % l, log_l, l)
        add("l%d:n=l+1" % l, log_l, l + 1)
    return out
