"""Numpy restatement of the on-device QAP pair generator (``graph_neural_net_amd/csrc/pairgen.hip``).

Test infrastructure only; the package never imports it.  The same algorithms on the same counter-based streams,
written plainly, so that the device output can be compared with it bit for bit:

* randomness: Philox4x64-10 keyed by (seed, 0).  Raw 32-bit draw ``t`` of stream ``s`` of pair ``k`` is 32-bit word
  ``t & 7`` (low half first) of the block at counter (t >> 3, k, s, 0).  ``philox4x64`` is checked against
  ``numpy.random.Philox`` by ``tests/test_pairgen_host.py``;
* a probability ``x`` is the integer threshold ``min(2**32, floor(x * 2**32))`` and an event is ``u32 < thr``;
  an integer in [0, k) is ``(u32 * k) >> 32``.  No float is compared anywhere.
"""
import math

import numpy as np

STREAM_SIZE, STREAM_PARENT, STREAM_NOISE1, STREAM_NOISE2, STREAM_RELABEL, STREAM_CHAIN = range(6)
FAMILIES = {'ErdosRenyi': 0, 'Regular': 1, 'BarabasiAlbert': 2}
NOISE_MODELS = {'ErdosRenyi': 0, 'EdgeSwap': 1}
MAX_SIZE_DRAWS = 64          # n_i < 2 is redrawn at most this often; after that n_i = 2

_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)
_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)
_PHILOX_M = (np.uint64(0xD2E7470EE14C6C93), np.uint64(0xCA5A826395121157))
_PHILOX_W = (0x9E3779B97F4A7C15, 0xBB67AE8584CAA73B)


def threshold(x):
    return min(1 << 32, int(math.floor(x * 4294967296.0)))


def _mulhilo(a, b):
    """64 x 64 -> (hi, lo) on uint64 arrays, by 32-bit halves."""
    a0, a1 = a & _M32, a >> _S32
    b0, b1 = b & _M32, b >> _S32
    p00, p01, p10, p11 = a0 * b0, a0 * b1, a1 * b0, a1 * b1
    mid = (p00 >> _S32) + (p01 & _M32) + (p10 & _M32)
    hi = p11 + (p01 >> _S32) + (p10 >> _S32) + (mid >> _S32)
    return hi, a * b


def philox4x64(ctr, key):
    """ctr: (4, K) uint64 array of counters, key: two ints -> (4, K) uint64 outputs (Random123's Philox4x64-10)."""
    c = [np.asarray(x, dtype=np.uint64).copy() for x in ctr]
    k0, k1 = int(key[0]) & 0xFFFFFFFFFFFFFFFF, int(key[1]) & 0xFFFFFFFFFFFFFFFF
    with np.errstate(over='ignore'):
        for r in range(10):
            if r:
                k0 = (k0 + _PHILOX_W[0]) & 0xFFFFFFFFFFFFFFFF
                k1 = (k1 + _PHILOX_W[1]) & 0xFFFFFFFFFFFFFFFF
            hi0, lo0 = _mulhilo(_PHILOX_M[0], c[0])
            hi1, lo1 = _mulhilo(_PHILOX_M[1], c[2])
            c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
    return np.stack(c)


def draws(seed, pair, stream, pos):
    """Raw u32 draws (as int64) at the positions ``pos`` of one stream of one pair."""
    pos = np.asarray(pos, dtype=np.uint64).reshape(-1)
    q = pos >> np.uint64(3)
    ctr = [q, np.full_like(q, np.uint64(pair)), np.full_like(q, np.uint64(stream)), np.zeros_like(q)]
    out = philox4x64(ctr, (seed, 0))
    w = (pos & np.uint64(7)).astype(np.int64)
    word = out[w >> 1, np.arange(len(pos))]
    return ((word >> (np.uint64(32) * (w & 1).astype(np.uint64))) & _M32).astype(np.int64)


def below(u, k):
    """Integer in [0, k) from a u32 draw (multiply-shift)."""
    return (u * k) >> 32


def regular_degree(n, p):
    d = int(p * n)
    if (n * d) % 2 == 1:
        d += 1
    return d


def ba_attachments(n, p):
    return int(p * (n - 1) / 2)


def vertex_count(seed, k, N, thr_v):
    if thr_v >= 1 << 32:
        return N
    for r in range(MAX_SIZE_DRAWS):
        n = int((draws(seed, k, STREAM_SIZE, r * N + np.arange(N)) < thr_v).sum())
        if n >= 2:
            return n
    return 2


def _upper(n, N):
    i, j = np.triu_indices(n, 1)
    return i, j, i * N + j


def erdos_renyi(seed, k, stream, n, N, thr):
    w = np.zeros((n, n), dtype=bool)
    i, j, pos = _upper(n, N)
    e = draws(seed, k, stream, pos) < thr
    w[i[e], j[e]] = True
    return w | w.T


def random_regular(seed, k, n, d, swaps_per_edge):
    """Circulant seed (edge (k-1)*n + i = {i, i+k}, then {i, i+n/2} for odd d), swaps_per_edge * m double-edge swaps
    (synthetic.random_regular's scheme), random relabelling (Fisher-Yates from the top)."""
    w = np.zeros((n, n), dtype=bool)
    edges = []
    for s in range(1, d // 2 + 1):
        for i in range(n):
            edges.append((i, (i + s) % n))
    if d % 2:
        for i in range(n // 2):
            edges.append((i, i + n // 2))
    edges = [(min(u, v), max(u, v)) for u, v in edges]
    for u, v in edges:
        w[u, v] = w[v, u] = True
    m = len(edges)
    steps = swaps_per_edge * m
    if steps:
        u32 = draws(seed, k, STREAM_CHAIN, np.arange(4 * steps)).reshape(steps, 4)
        A, Bv, F = below(u32[:, 0], m), below(u32[:, 1], m), u32[:, 2] >> 31
        for a, b, f in zip(A.tolist(), Bv.tolist(), F.tolist()):
            if a == b:
                continue
            u, v = edges[a]
            s, t = edges[b]
            if f:
                s, t = t, s
            if u == t or s == v or u == s or v == t:
                continue
            if w[u, t] or w[s, v]:
                continue
            w[u, v] = w[v, u] = False
            w[s, t] = w[t, s] = False
            w[u, t] = w[t, u] = True
            w[s, v] = w[v, s] = True
            edges[a] = (min(u, t), max(u, t))
            edges[b] = (min(s, v), max(s, v))
    perm = np.arange(n)
    if n > 1:
        r = draws(seed, k, STREAM_RELABEL, np.arange(n))
        for i in range(n - 1, 0, -1):
            j = int(below(int(r[i]), i + 1))
            perm[i], perm[j] = perm[j], perm[i]
    return w[np.ix_(perm, perm)]


def barabasi_albert(seed, k, n, m):
    """networkx 3.x barabasi_albert_graph: a star on m + 1 nodes, then node `source` takes m distinct targets drawn from
    the repeated-nodes list (duplicates rejected); the list grows by the targets (in the order drawn) and m copies of source."""
    w = np.zeros((n, n), dtype=bool)
    w[0, 1:m + 1] = w[1:m + 1, 0] = True
    rep = [0] * m + list(range(1, m + 1))
    need = m * (n - m - 1)
    t, chunk, buf = 0, 0, np.zeros(0, dtype=np.int64)
    for source in range(m + 1, n):
        targets = []
        while len(targets) < m:
            if t >= chunk:
                buf = draws(seed, k, STREAM_CHAIN, np.arange(t, t + 4 * need + 64))
                base, chunk = t, t + len(buf)
            x = rep[below(int(buf[t - base]), len(rep))]
            t += 1
            if x not in targets:
                targets.append(x)
        for x in targets:
            w[source, x] = w[x, source] = True
        rep.extend(targets)
        rep.extend([source] * m)
    return w


def noise_erdos_renyi(seed, k, w, N, thr1, thr2):
    n = w.shape[0]
    i, j, pos = _upper(n, N)
    z1 = draws(seed, k, STREAM_NOISE1, pos) < thr1
    z2 = draws(seed, k, STREAM_NOISE2, pos) < thr2
    par = w[i, j]
    e = (par & ~z1) | (~par & z2)
    wn = np.zeros_like(w)
    wn[i[e], j[e]] = True
    return wn | wn.T


def noise_edge_swap(seed, k, w, thr):
    """loaders/data_generator.py:89-116 on the parent's edge list: the (u < v) edges in row-major order, then their
    reversals.  Outer draw o (stream noise-1), inner draw o * 2m + i (stream noise-2); after a swap (u, v) is gone, so
    at most one swap per outer edge."""
    iu, ju = np.nonzero(np.triu(w, 1))
    el = list(zip(iu.tolist(), ju.tolist()))
    el = el + [(v, u) for u, v in el]
    L = len(el)
    g = w.copy()
    if L == 0:
        return g
    fire = np.nonzero(draws(seed, k, STREAM_NOISE1, np.arange(L)) < thr)[0]
    for o in fire.tolist():
        u, v = el[o]
        if not g[u, v]:
            continue
        cand = np.nonzero(draws(seed, k, STREAM_NOISE2, o * L + np.arange(L)) < thr)[0]
        for i in cand.tolist():
            s, t = el[i]
            if g[s, t] and u != t and s != v and not g[u, t] and not g[s, v]:
                g[u, v] = g[v, u] = g[s, t] = g[t, s] = False
                g[u, t] = g[t, u] = g[s, v] = g[v, s] = True
                break
    return g


def generate_pair(seed, k, N, family, noise_model, p, noise, vertex_proba=1.0, swaps_per_edge=10):
    """Pair k of dataset `seed`: (W, W_noise) as (N, N) bool (zero outside n), and n."""
    n = vertex_count(seed, k, N, threshold(vertex_proba))
    if family == 'ErdosRenyi':
        w = erdos_renyi(seed, k, STREAM_PARENT, n, N, threshold(p))
    elif family == 'Regular':
        w = random_regular(seed, k, n, regular_degree(n, p), swaps_per_edge)
    elif family == 'BarabasiAlbert':
        w = barabasi_albert(seed, k, n, ba_attachments(n, p))
    else:
        raise ValueError('unknown graph family %r' % (family,))
    if noise_model == 'ErdosRenyi':
        wn = noise_erdos_renyi(seed, k, w, N, threshold(noise), threshold(p * noise / (1 - p)))
    elif noise_model == 'EdgeSwap':
        wn = noise_edge_swap(seed, k, w, threshold(noise))
    else:
        raise ValueError('unknown noise model %r' % (noise_model,))
    W = np.zeros((N, N), dtype=bool)
    Wn = np.zeros((N, N), dtype=bool)
    W[:n, :n] = w
    Wn[:n, :n] = wn
    return W, Wn, n


def generate(seed, first, count, N, family='Regular', noise_model='ErdosRenyi', p=0.2, noise=0.1, vertex_proba=1.0,
             swaps_per_edge=10):
    """Pairs first .. first + count - 1: (W1, W2) as (count, N, N) bool and n as (count,) int."""
    out = [generate_pair(seed, first + c, N, family, noise_model, p, noise, vertex_proba, swaps_per_edge) for c in range(count)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.array([o[2] for o in out], dtype=np.int64)
