"""NumPy twin of the ragged plan's packed row order (matcha_amd/csrc/ragged.hip: row_scan_kernel's schedule, row_fill_kernel's destinations) and
of the greedy half-tile packer that runs on top of it (ragged_roles.hpp: tile_pack_wave).  Integer arithmetic only, written to give the SAME
numbers as the kernels: tests/test_hip_row_pack.py compares the device's arrays with these bit for bit, tests/test_cpu_row_pack.py checks the
order's properties without a GPU.

The order.  Rows fall into classes by their number of real tokens k = 0 .. 8.  A SCHEDULE is a short list of phases; a phase is a recipe a_k
(rows of class k per half tile, sum k a_k <= 31) repeated over m tiles, and it ends when a class cannot fill another tile.  Inside a tile the
classes stand in ascending order.  The last phase holds whatever is left, class by class.  Row r of class k (r counts the class's rows in batch
order) therefore has its plan row and its first token in closed form."""
import numpy as np

MAX_L = 8
NCLS = MAX_L + 1
HALF_TOK = 31
SUPER_TOK = 63 * 32
MAX_PHASES = 12
TAIL_TOK = 64 * HALF_TOK         # at most this many tokens left (or 1 / 32 of the batch's): the remaining rows go in class order


def _recipe(rem):
    """Rows per class of one half tile: the classes' shares of the remaining tokens rounded down, the slots left filled exactly by a bounded
    knapsack over what remains (classes 8 .. 1)."""
    T = sum(c * rem[c] for c in range(1, NCLS))
    s = 0
    while (T >> s) >= (1 << 26):
        s += 1
    Ts = sum(c * (rem[c] >> s) for c in range(1, NCLS))
    a = [0] * NCLS
    for c in range(1, NCLS):
        a[c] = min(rem[c], (HALF_TOK * (rem[c] >> s)) // Ts) if Ts > 0 else 0
    left = HALF_TOK - sum(c * a[c] for c in range(1, NCLS))
    reach, before = 1, [0] * NCLS
    for c in range(MAX_L, 0, -1):
        before[c] = reach
        for _ in range(min(rem[c] - a[c], left // c)):
            reach |= reach << c
        reach &= (1 << (left + 1)) - 1
    w = reach.bit_length() - 1
    for c in range(1, NCLS):
        j = 0
        while not (before[c] >> (w - j * c)) & 1:
            j += 1
        a[c] += j
        w -= j * c
    return a


def schedule(n):
    """n[k]: rows of class k.  Phases as dicts of plain ints / lists."""
    rem = [int(v) for v in n]
    assert len(rem) == NCLS
    phases, row_base, tok_base, cls_base, pred_k = [], 0, 0, [0] * NCLS, 0
    tail_tok = max(TAIL_TOK, sum(c * rem[c] for c in range(1, NCLS)) >> 5)
    while sum(rem) > 0:
        T = sum(c * rem[c] for c in range(1, NCLS))
        last = len(phases) == MAX_PHASES - 1 or T <= tail_tok
        if last:
            a, m = list(rem), 1
        else:
            a = _recipe(rem)
            m = min(rem[c] // a[c] for c in range(1, NCLS) if a[c] > 0)
            a[0] = rem[0] // m
        row_in, tok_in, prev_k, r_acc, t_acc, pk = [0] * NCLS, [0] * NCLS, [-1] * NCLS, 0, 0, -1
        for c in range(NCLS):
            row_in[c], tok_in[c], prev_k[c] = r_acc, t_acc, pk
            r_acc += a[c]
            t_acc += c * a[c]
            if a[c] > 0:
                pk = c
        phases.append(dict(m=m, a=a, row_in=row_in, tok_in=tok_in, prev_k=prev_k, rows=r_acc, toks=t_acc, row_base=row_base, tok_base=tok_base,
                           cls_base=list(cls_base), pred_k=pred_k, last_k=pk))
        for c in range(NCLS):
            rem[c] -= m * a[c]
            cls_base[c] += m * a[c]
        row_base += m * r_acc
        tok_base += m * t_acc
        pred_k = pk
        if last:
            break
    return phases


def destinations(k, phases):
    """k[b]: class of batch row b.  -> (plan row, first token, k of the plan row in front) per batch row."""
    k = np.asarray(k, dtype=np.int64)
    B = len(k)
    rank = np.zeros(B, dtype=np.int64)
    for c in range(NCLS):
        sel = k == c
        rank[sel] = np.arange(int(sel.sum()))
    dst, pos, kprev = np.zeros(B, np.int64), np.zeros(B, np.int64), np.zeros(B, np.int64)
    base = np.array([p["cls_base"] for p in phases], dtype=np.int64).reshape(len(phases), NCLS)
    for b in range(B):
        c, r = int(k[b]), int(rank[b])
        p = int(np.nonzero(base[:, c] <= r)[0][-1])
        ph = phases[p]
        q = r - ph["cls_base"][c]
        t, j = divmod(q, ph["a"][c])
        dst[b] = ph["row_base"] + t * ph["rows"] + ph["row_in"][c] + j
        pos[b] = ph["tok_base"] + t * ph["toks"] + ph["tok_in"][c] + j * c
        kprev[b] = c if j > 0 else ph["prev_k"][c] if ph["prev_k"][c] >= 0 else ph["last_k"] if t > 0 else ph["pred_k"]
    return dst, pos, kprev


def half_tiles(row_off, sb_first, B):
    """tile_pack_wave over every planning superblock, half tiles: [first token, tokens, first row, rows]."""
    out = []
    nsb = len(sb_first) - 1
    for s in range(nsb):
        b_lo, b_hi = int(sb_first[s]), B
        for q in range(s + 1, nsb):
            if sb_first[q] < B:
                b_hi = int(sb_first[q])
                break
        if b_lo >= b_hi:
            continue
        tile_b0, tile_tok0 = b_lo, int(row_off[b_lo])
        for b in range(b_lo, b_hi):
            if row_off[b + 1] - tile_tok0 > HALF_TOK:
                out.append((tile_tok0, int(row_off[b]) - tile_tok0, tile_b0, b - tile_b0))
                tile_b0, tile_tok0 = b, int(row_off[b])
        out.append((tile_tok0, int(row_off[b_hi]) - tile_tok0, tile_b0, b_hi - tile_b0))
    return np.array(out, dtype=np.int32).reshape(-1, 4)


def plan(x, n_nodes=None, packed=True):
    """The plan of batch x [B, L] (0 = padding): row_src, row_off, the token lists, sb_first, the half tiles and count[1], count[3]."""
    x = np.asarray(x, dtype=np.int64)
    B, L = x.shape
    assert 1 <= L <= MAX_L
    real = x != 0
    k = real.sum(1)
    if packed:
        phases = schedule(np.bincount(k, minlength=NCLS))
        dst, pos, kprev = destinations(k, phases)
    else:
        phases = []
        dst = np.arange(B, dtype=np.int64)
        pos = np.concatenate([[0], np.cumsum(k)[:-1]])
        kprev = np.concatenate([[0], k[:-1]])
    Tr, T = int(k.sum()), B * L
    row_src = np.zeros(B, np.int32)
    row_src[dst] = np.arange(B, dtype=np.int32)
    row_off = np.zeros(B + 1, np.int32)
    row_off[dst] = pos
    row_off[B] = Tr
    tok_slot, tok_id, tok_key, tok_pos = np.zeros(T + 1, np.int32), np.zeros(T + 1, np.int64), np.zeros(T + 1, np.int32), np.zeros(T + 1, np.int32)
    ids = x.copy()
    if n_nodes is not None:
        ids[(ids < 0) | (ids > n_nodes)] = 0
    nth = np.cumsum(real, axis=1) - 1
    bb, ll = np.nonzero(real)
    at = pos[bb] + nth[bb, ll]
    tok_slot[at] = bb * L + ll
    tok_id[at] = ids[bb, ll]
    tok_key[at] = ids[bb, ll]
    tok_pos[at] = nth[bb, ll] | (k[bb] << 8)
    tok_slot[Tr] = B * L
    nsb = -(-(T + 1) // SUPER_TOK)
    sb_first = np.full(nsb + 1, B, np.int32)
    mark = (dst == 0) | (pos // SUPER_TOK != (pos - kprev) // SUPER_TOK)
    sb_first[pos[mark] // SUPER_TOK] = dst[mark]
    tiles = half_tiles(row_off, sb_first, B)
    return dict(row_src=row_src, row_off=row_off, tok_slot=tok_slot, tok_id=tok_id, tok_key=tok_key, tok_pos=tok_pos, sb_first=sb_first, half_meta=tiles,
                tokens=Tr, halves=len(tiles), phases=phases, k=k)
