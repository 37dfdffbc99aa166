"""Distribution statistics of generated QAP pairs, shared by tests/golden/make_pairgen_stats.py (the reference's own generators)
and the tests of the on-device generator (its numpy restatement on the host, the device at large K)."""
import numpy as np
import torch

_BASE = dict(n_vertices=50, generative_model='Regular', noise_model='ErdosRenyi', edge_density=0.2, noise=0.1, vertex_proba=1.0)
CONFIGS = {
    'regular_er_n50': dict(_BASE),
    'regular_edgeswap_n50': dict(_BASE, noise_model='EdgeSwap'),
    'er_er_n50': dict(_BASE, generative_model='ErdosRenyi'),
    'ba_er_n50': dict(_BASE, generative_model='BarabasiAlbert'),
    'regular_er_n200': dict(_BASE, n_vertices=200),
    'er_er_n50_vp08': dict(_BASE, generative_model='ErdosRenyi', vertex_proba=0.8),
}
STATS = ('edges', 'degree_var', 'triangles', 'shared_edges', 'max_degree', 'n')


def statistics(a1, a2, n=None):
    """a1, a2: (K, N, N) 0/1 float64 tensors (zero outside n); n: (K,) vertex counts or None -> {stat: (K,) tensor}."""
    K, N = a1.shape[0], a1.shape[-1]
    if n is None:
        n = torch.full((K,), float(N), dtype=a1.dtype, device=a1.device)
    deg = a1.sum(-1)
    valid = torch.arange(N, device=a1.device)[None, :] < n[:, None]
    mean = deg.sum(-1) / n
    var = (((deg - mean[:, None]) ** 2) * valid).sum(-1) / n
    return {
        'edges': a1.sum((1, 2)) / 2,
        'degree_var': var,
        'triangles': torch.einsum('kij,kjl,kli->k', a1, a1, a1) / 6,
        'shared_edges': (a1 * a2).sum((1, 2)) / 2,
        'max_degree': deg.max(-1).values,
        'n': n.clone(),
    }


def summarize(name, st):
    """{stat: (K,) array} -> fixture entries '<config>/<stat>' = [mean, std, K]."""
    return {'%s/%s' % (name, k): np.array([np.mean(v), np.std(v), len(v)], dtype=np.float64) for k, v in st.items()}


def gate_failures(fixture, name, st):
    """Statistics whose mean is off the fixture's by more than 4 sqrt(s_ref^2 / K_ref + s^2 / K) -> list of messages."""
    bad = []
    for k in STATS:
        m_ref, s_ref, k_ref = fixture['%s/%s' % (name, k)]
        v = np.asarray(st[k], dtype=np.float64)
        d = abs(v.mean() - m_ref)
        gate = 4 * np.sqrt(s_ref ** 2 / k_ref + v.std() ** 2 / len(v)) + 1e-9 * (1 + abs(m_ref))
        if d > gate:
            bad.append('%s %s: mean %.4f vs reference %.4f (gate %.4f)' % (name, k, v.mean(), m_ref, gate))
    return bad
