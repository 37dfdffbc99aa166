"""CPU: the host side of planted permutations -- the host route of the metrics and decoders with ``labels=`` against the restatement
of the reference's loops (tests/planted_ref.py) and against the outputs recorded from the reference (tests/golden/planted_labels.npz),
``planted.inverse``, and argument validation."""
import numpy as np
import pytest
import torch

import planted_ref as R
from graph_neural_net_amd import planted, qap
from graph_neural_net_amd.masked import MaskedTensor
from graph_neural_net_amd.metrics import accuracy_linear_assignment, accuracy_max
from graph_neural_net_amd.pairgen import PairGenerator
from util import load_golden, sub

GROUPS = ('rand5', 'rand64', 'ties8', 'const7', 'ragged12', 'ragged_const65')


def _perms(rng, sizes, N):
    lab = np.full((len(sizes), N), -1, dtype=np.int32)
    for b, n in enumerate(sizes):
        lab[b, :n] = rng.permutation(n)
    return lab


def _scores(kind, rng, B, N):
    if kind == 'random':
        return (3 * rng.standard_normal((B, N, N))).astype(np.float32)
    if kind == 'ties':
        return rng.integers(0, 3, (B, N, N)).astype(np.float32)
    return np.full((B, N, N), 0.25, dtype=np.float32)


def _batch(s, sizes, N):
    """scores as the metrics take them: a plain tensor for a constant-size batch, else a MaskedTensor with zeros in the padding"""
    if all(n == N for n in sizes):
        return torch.from_numpy(s)
    t = torch.from_numpy(s).clone()
    for b, n in enumerate(sizes):
        t[b, n:, :] = 0
        t[b, :, n:] = 0
    return MaskedTensor(t, torch.tensor(sizes, dtype=torch.int32), (1, 2), 'N')


@pytest.mark.parametrize('kind', ['random', 'ties', 'const'])
@pytest.mark.parametrize('N', [1, 5, 64, 65, 100])
def test_host_metrics_with_labels_equal_the_reference_loop(N, kind):
    rng = np.random.default_rng(10 * N + len(kind))
    for sizes in ([N, N, N], [N, max(1, N // 2), max(1, N - 1)]):
        s = _scores(kind, rng, len(sizes), N)
        lab = _perms(rng, sizes, N)
        x = _batch(s, sizes, N)
        raw = x.tensor if isinstance(x, MaskedTensor) else x
        for fn, ref in ((accuracy_linear_assignment, R.lsap_counts), (accuracy_max, R.max_counts)):
            want = ref(raw, sizes, lab)
            assert fn(x, labels=torch.from_numpy(lab)) == (sum(want), sum(sizes))
            assert fn(x, aggregate_score=False, labels=torch.from_numpy(lab)) == [c / n for c, n in zip(want, sizes)]
            # the reference's form: a list of per-graph arrays
            assert fn(x, labels=[lab[b, :n] for b, n in enumerate(sizes)]) == (sum(want), sum(sizes))
            # labels=None is the identity
            assert fn(x) == fn(x, labels=torch.arange(N).expand(len(sizes), N)) == (sum(ref(raw, sizes)), sum(sizes))


def test_constant_scores_count_every_vertex_and_with_labels_the_fixed_points():
    rng = np.random.default_rng(3)
    B, N = 5, 23
    s = torch.full((B, N, N), 0.5)
    lab = _perms(rng, [N] * B, N)
    lab[0] = np.arange(N)
    fixed = int((lab == np.arange(N)).sum())
    assert accuracy_linear_assignment(s) == (B * N, B * N)
    assert accuracy_linear_assignment(s, labels=torch.from_numpy(lab)) == (fixed, B * N)
    assert 0 < fixed < B * N


@pytest.mark.parametrize('name', GROUPS)
def test_host_metrics_reproduce_the_recorded_reference_outputs(name):
    g = sub(load_golden('planted_labels.npz'), name + '/')
    sizes = g['nvalid'].tolist()
    N = g['scores'].shape[1]
    x = _batch(g['scores'].numpy(), sizes, N)
    for fn, key in ((accuracy_linear_assignment, 'lsap'), (accuracy_max, 'max')):
        assert fn(x, labels=g['labels']) == (int(g[key + '_correct'].sum()), sum(sizes))
        assert fn(x, aggregate_score=False, labels=g['labels']) == g[key + '_acc'].tolist()
        assert fn(x, labels=[g['labels'][b, :n].numpy() for b, n in enumerate(sizes)]) == (int(g[key + '_correct'].sum()), sum(sizes))
    # the restatement is the reference's loop
    raw = x.tensor if isinstance(x, MaskedTensor) else x
    assert R.lsap_counts(raw, sizes, g['labels'].numpy()) == g['lsap_correct'].tolist()
    assert R.max_counts(raw, sizes, g['labels'].numpy()) == g['max_correct'].tolist()


def _pairs(rng, sizes, N, weighted):
    """symmetric A, a non-symmetric B; 0/1 words, or dyadic weights k / 8 as (B, N, N) float32"""
    As, Bs = np.zeros((len(sizes), N, N)), np.zeros((len(sizes), N, N))
    for b, n in enumerate(sizes):
        a = np.triu(rng.random((n, n)) < 0.4, 1)
        As[b, :n, :n] = a | a.T
        Bs[b, :n, :n] = (As[b, :n, :n] > 0) & (rng.random((n, n)) < 0.8)
        if weighted:
            As[b, :n, :n] *= rng.integers(1, 8, (n, n)) / 8
            Bs[b, :n, :n] *= rng.integers(1, 8, (n, n)) / 8
    if weighted:
        return As, Bs, torch.from_numpy(As).float(), torch.from_numpy(Bs).float()
    to_words = lambda M: torch.from_numpy(R.pack_bits(M.astype(np.uint8)).view(np.int32))
    return As, Bs, to_words(As), to_words(Bs)


@pytest.mark.parametrize('weighted', [False, True])
def test_host_decoders_with_labels_equal_the_reference_loops(weighted):
    rng = np.random.default_rng(40 + weighted)
    N, sizes = 12, [12, 7, 1, 10]
    As, Bs, x1, x2 = _pairs(rng, sizes, N, weighted)
    lab = _perms(rng, sizes, N)
    nv = torch.tensor(sizes, dtype=torch.int32)
    s = torch.from_numpy((2 * rng.standard_normal((len(sizes), N, N))).astype(np.float32))
    acc, q, planted_obj = qap.all_acc_qap(s, x1, x2, nvalid=nv, weighted=weighted, labels=torch.from_numpy(lab))
    want = R.all_acc_qap(s, As, Bs, sizes, lab)
    for got, ref in zip((acc, q, planted_obj), want):
        assert np.array_equal(got.numpy().astype(np.float64), ref.astype(np.float64))
    assert np.array_equal(planted_obj.numpy(), qap.qap_objective(x1, x2, torch.from_numpy(lab), nvalid=nv, weighted=weighted)['qap'].numpy())
    # labels=None changes nothing
    for a, b in zip(qap.all_acc_qap(s, x1, x2, nvalid=nv, weighted=weighted), qap.all_acc_qap(s, x1, x2, nv, weighted, None)):
        assert torch.equal(a, b)
    start = _perms(rng, sizes, N)
    for T in (0, 1, 3):
        out = qap.greedy_qap(x1, x2, torch.from_numpy(start), T, nv, weighted=weighted, labels=torch.from_numpy(lab))
        plain = qap.greedy_qap(x1, x2, torch.from_numpy(start), T, nv, weighted=weighted)
        for b, n in enumerate(sizes):
            s_best, acc_best, t_best = R.greedy_qap(As[b, :n, :n], Bs[b, :n, :n], start[b, :n], T, lab[b, :n])
            assert (float(out['s_best'][b]), int(out['acc_best'][b]), int(out['T_best'][b])) == (s_best, acc_best, t_best)
        for k in ('s_best', 'na', 'nb', 'T_best', 'perm'):              # only acc_best knows the labels
            assert torch.equal(out[k], plain[k])


def test_inverse():
    rng = np.random.default_rng(5)
    sizes = [9, 1, 0, 6, 9]
    lab = torch.from_numpy(_perms(rng, sizes, 9))
    inv = planted.inverse(lab)
    assert inv.dtype == lab.dtype and inv.shape == lab.shape
    for b, n in enumerate(sizes):
        assert np.array_equal(inv[b, :n].numpy(), R.inverse(lab[b].numpy(), n))
        assert (inv[b, n:] == -1).all()
        assert torch.equal(lab[b, inv[b, :n].long()], torch.arange(n, dtype=lab.dtype))
    assert torch.equal(planted.inverse(inv), lab)
    assert torch.equal(planted.inverse(lab.long()), inv.long())
    with pytest.raises(ValueError):
        planted.inverse(lab.float())
    with pytest.raises(ValueError):
        planted.inverse(lab[0])


def test_labels_are_validated():
    s = torch.zeros(2, 4, 4)
    ok = torch.arange(4).expand(2, 4)
    for fn in (accuracy_linear_assignment, accuracy_max):
        for bad in (ok[:1], ok[:, :3], ok.float(), ok[0], [np.arange(4)], [np.arange(5), np.arange(4)], [np.arange(4.0), np.arange(4)]):
            with pytest.raises(ValueError):
                fn(s, labels=bad)
    bits = torch.zeros(2, 4, 1, dtype=torch.int32)
    with pytest.raises(ValueError):
        qap.all_acc_qap(s, bits, bits, labels=ok[:, :3])
    with pytest.raises(ValueError):
        qap.greedy_qap(bits, bits, ok.int(), 1, labels=ok.float())
    # relabelling and drawing run on the GPU only
    with pytest.raises(RuntimeError, match='GPU only'):
        planted.relabel(bits, ok.int())
    with pytest.raises(RuntimeError, match='GPU only'):
        planted.relabel({'input': torch.zeros(2, 2, 4, 4)}, ok.int())
    with pytest.raises(RuntimeError, match='GPU only'):
        planted.planted_permutation(0, 4, 0, 2, device='cpu')
    with pytest.raises(ValueError):
        planted.planted_permutation(0, 257, 0, 2, device='cpu')


@pytest.mark.parametrize('form', ['bits', 'dense', 'spectral'])
def test_permute_on_a_cpu_generator_raises_the_gpu_only_message(form):
    gen = PairGenerator(10, 'ErdosRenyi', device='cpu')
    with pytest.raises(RuntimeError, match='GPU only'):
        getattr(gen, form)(0, 2, permute=True)
