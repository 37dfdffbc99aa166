"""GPU: planted permutations (csrc/planted.hip, graph_neural_net_amd/planted.py, PairGenerator(..., permute=True)) and the label-taking
metrics and decoders, against the numpy restatement tests/planted_ref.py and the reference's recorded outputs
(tests/golden/planted_labels.npz).  Everything but the end-to-end scores is integer arithmetic or data movement: exact equality.
"""
import functools

import numpy as np
import pytest
import torch

import planted_ref as R
import spectral_ref as SR
from graph_neural_net_amd import planted, qap, synthetic
from graph_neural_net_amd.inputs import expand_adjacency
from graph_neural_net_amd.masked import MaskedTensor, from_list
from graph_neural_net_amd.metrics import accuracy_linear_assignment, accuracy_max, lsap_device
from graph_neural_net_amd.pairgen import PairGenerator
from graph_neural_net_amd.siamese import Siamese_Node_Exp
from oracle import fgnn_oracle as O
from test_gpu_parity import E2E_FWD_TOL
from test_gpu_spectral import ERR_GATE
from util import load_golden, rel, sub

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SEEDS = (11, (1 << 40) + 5)


def _dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(DEV)


def _perms(rng, sizes, N):
    lab = np.full((len(sizes), N), -1, dtype=np.int32)
    for b, n in enumerate(sizes):
        lab[b, :n] = rng.permutation(n)
    return lab


def _is_perm_rows(lab, sizes):
    return all(np.array_equal(np.sort(lab[b, :n]), np.arange(n)) and (lab[b, n:] == -1).all() for b, n in enumerate(sizes))


# ---- 1. planted_permutation ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', SEEDS)
@pytest.mark.parametrize('N,vp', [(N, vp) for N in (1, 2, 3, 31, 32, 33, 64, 65, 200, 256) for vp in (1.0, 0.7) if N > 1 or vp == 1.0])
def test_planted_permutation_is_bit_equal_to_the_restatement(N, vp, seed):
    count = 40
    nv = None if vp == 1.0 else PairGenerator(N, 'ErdosRenyi', vertex_proba=vp, seed=seed, device=DEV).bits(0, count)[2]
    sizes = [N] * count if nv is None else nv.tolist()
    want = R.planted_labels(seed, range(count), N, sizes)
    got = planted.planted_permutation(seed, N, 0, count, nvalid=nv, device=DEV)
    assert got.shape == (count, N) and got.dtype == torch.int32 and got.is_cuda
    assert _is_perm_rows(got.cpu().numpy(), sizes)
    assert np.array_equal(got.cpu().numpy(), want)
    # pair k depends on (seed, k) only: a split range, an index list in any order, duplicates
    cut = lambda a, b: None if nv is None else nv[a:b]
    parts = [planted.planted_permutation(seed, N, 0, 17, nvalid=cut(0, 17), device=DEV),
             planted.planted_permutation(seed, N, 17, 23, nvalid=cut(17, 40), device=DEV)]
    assert torch.equal(torch.cat(parts), got)
    order = torch.from_numpy(np.random.default_rng(N).permutation(count)).to(DEV)
    shuffled = planted.planted_permutation(seed, N, index=order, nvalid=None if nv is None else nv[order], device=DEV)
    assert torch.equal(shuffled, got[order])
    assert torch.equal(planted.planted_permutation(seed, N, index=torch.arange(count), nvalid=nv, device=DEV), got)
    dup = torch.tensor([5, 5, 39, -1, 5], device=DEV)
    nvd = None if nv is None else nv[dup.clamp(min=0)]
    rows = planted.planted_permutation(seed, N, index=dup, nvalid=nvd, device=DEV)
    assert torch.equal(rows[0], got[5]) and torch.equal(rows[1], got[5]) and torch.equal(rows[4], got[5]) and torch.equal(rows[2], got[39])
    assert (rows[3] == -1).all()                                  # a negative index: the empty permutation
    if N >= 31 and nv is None:
        assert not torch.equal(got, planted.planted_permutation(seed + 1, N, 0, count, device=DEV))
        assert int((got == torch.arange(N, device=DEV)).sum()) < count * N // 4


# ---- 2. relabel on bit words ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', [1, 31, 32, 33, 63, 64, 65, 96, 97, 255, 256])
def test_relabel_bits_equals_the_index_expression(N):
    rng = np.random.default_rng(200 + N)
    B = 4
    M = (rng.random((B, N, N)) < 0.4).astype(np.uint8)                  # not symmetric
    clean = R.pack_bits(M)
    for sizes in ([N] * B, [N, max(1, N // 2), 0, max(1, N - 1)]):
        lab = _perms(rng, sizes, N)
        ragged = sizes != [N] * B
        words = clean
        if ragged:                                                      # all-ones garbage outside every corner, padding bits included
            full = np.ones((B, N, 32 * clean.shape[2]), dtype=np.uint8)
            for b, n in enumerate(sizes):
                full[b, :n, :n] = M[b, :n, :n]
            words = np.packbits(full, axis=-1, bitorder='little').view(np.uint32).reshape(clean.shape)
        nv = _dev(np.asarray(sizes, dtype=np.int32)) if ragged else None
        got = planted.relabel(_dev(words), _dev(lab), nv)
        assert got.dtype == torch.int32 and got.shape == (B, N, clean.shape[2])
        want = R.relabel_bits(clean, lab, sizes)
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want)
        for b, n in enumerate(sizes):                                   # W[np.ix_(inv, inv)], zeros outside the corner
            inv = R.inverse(lab[b], n)
            out = R.unpack_bits(want[b:b + 1], N)[0]
            assert np.array_equal(out[:n, :n], M[b, :n, :n][np.ix_(inv, inv)]) and out[n:].sum() == 0 and out[:, n:].sum() == 0
        back = planted.relabel(got, planted.inverse(_dev(lab)), nv)
        assert np.array_equal(back.cpu().numpy().view(np.uint32), R.relabel_bits(clean, np.tile(np.arange(N, dtype=np.int32), (B, 1)), sizes))


# ---- 3. relabel on dense tensors -----------------------------------------------------------------------------------------------
def _index_expression(x, lab, sizes):
    out = torch.zeros_like(x)
    for b, n in enumerate(sizes):
        inv = torch.from_numpy(R.inverse(lab[b], n)).to(x.device)
        out[b, :, :n, :n] = x[b, :, :n, :n][:, inv][:, :, inv]
    return out


@pytest.mark.parametrize('C', [1, 2, 4])
@pytest.mark.parametrize('N', [1, 17, 50, 64, 65, 200])
def test_relabel_dense_is_torch_equal_to_the_index_expression(N, C):
    rng = np.random.default_rng(300 + 10 * N + C)
    B = 3
    x = torch.from_numpy(rng.standard_normal((B, C, N, N)).astype(np.float32)).to(DEV)       # not symmetric
    lab = _perms(rng, [N] * B, N)
    got = planted.relabel(x, _dev(lab))
    assert torch.equal(got, _index_expression(x, lab, [N] * B))
    as_dict = planted.relabel({'input': x, 'other': 1}, _dev(lab))
    assert isinstance(as_dict, dict) and as_dict['other'] == 1 and torch.equal(as_dict['input'], got)
    assert torch.equal(planted.relabel(x[:, 0], _dev(lab)), got[:, 0])
    # a MaskedTensor cropped to its largest graph, labels at the generator's width, NaN in the input's padding
    sizes = [max(1, N - 3), max(1, N // 2), 1]
    m, wide = max(sizes), N + 5 if N + 5 <= 256 else N
    lab = np.full((B, wide), -1, dtype=np.int32)
    lab[:, :N] = _perms(rng, sizes, N)
    xm = x[:, :, :m, :m].clone()
    for b, n in enumerate(sizes):
        xm[b, :, n:, :] = float('nan')
        xm[b, :, :, n:] = float('nan')
    mt = MaskedTensor(xm, torch.tensor(sizes, dtype=torch.int32, device=DEV), (2, 3), 'M')
    out = planted.relabel(mt, _dev(lab))
    assert isinstance(out, MaskedTensor) and out.names == mt.names and out.masked_dims == mt.masked_dims and out.base_name == 'M'
    assert torch.equal(out.nvalid, mt.nvalid)
    assert torch.equal(out.tensor, _index_expression(torch.nan_to_num(xm), lab, sizes))
    back = planted.relabel(out, planted.inverse(_dev(lab)))
    assert torch.equal(back.tensor, torch.nan_to_num(xm))


@pytest.mark.parametrize('vp', [1.0, 0.7])
def test_relabelling_a_tensor_representation_is_the_representation_of_the_relabelled_graph(vp):
    gen = PairGenerator(50, 'Regular', 'ErdosRenyi', vertex_proba=vp, seed=9, device=DEV)
    b1, b2, nv = gen.bits(3, 5)
    lab = planted.planted_permutation(9, 50, 3, 5, nvalid=nv, device=DEV)
    assert torch.equal(expand_adjacency(planted.relabel(b2, lab, nv), 50, nv), planted.relabel(expand_adjacency(b2, 50, nv), lab, nv))
    # ... which is what permute=True hands out, side 1 and the unpermuted call untouched
    p1, p2, pnv, plab = gen.bits(3, 5, permute=True)
    assert torch.equal(p1, b1) and torch.equal(plab, lab) and torch.equal(p2, planted.relabel(b2, lab, nv))
    assert (nv is None and pnv is None) or torch.equal(pnv, nv)
    assert len(gen.bits(3, 5)) == 3 and len(gen.dense(3, 5)) == 2 and len(gen.spectral(3, 5)) == 2
    d1, d2, dlab = gen.dense(3, 5, permute=True)
    u1, u2 = gen.dense(3, 5)
    t = (lambda z: z['input']) if vp == 1.0 else (lambda z: z.tensor)
    assert torch.equal(dlab, lab) and torch.equal(t(d1), t(u1)) and torch.equal(t(d2), t(planted.relabel(u2, lab)))
    idx = torch.tensor([7, 3, 3, 5], device=DEV)
    i1, i2, inv_, ilab = gen.bits(index=idx, permute=True)
    assert torch.equal(ilab[1], lab[0]) and torch.equal(ilab[2], lab[0]) and torch.equal(ilab[3], lab[2]) and torch.equal(i2[1], p2[0])


# ---- 4. spectral(permute=True) -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('vp', [1.0, 0.7])
def test_spectral_of_a_permuted_pair(vp):
    N, P, count = 40, 4, 4
    gen = PairGenerator(N, 'ErdosRenyi', 'ErdosRenyi', edge_density=0.25, noise=0.1, vertex_proba=vp, seed=5, device=DEV)
    s1, s2, lab = gen.spectral(2, count, permute=True)
    u1, u2 = gen.spectral(2, count)
    b1, b2p, nv, lab2 = gen.bits(2, count, permute=True)
    assert torch.equal(lab, lab2)
    t = (lambda z: z['input']) if vp == 1.0 else (lambda z: z.tensor)
    assert torch.equal(t(s1), t(u1))
    got = t(s2)
    assert torch.equal(got[:, 0], t(planted.relabel(u2, lab))[:, 0])          # channel 0: one rounded product per entry, moved
    # higher powers: the gate of tests/test_gpu_spectral.py against the fp64 formula on the relabelled bit rows
    words = b2p.cpu().numpy().view(np.uint32)
    sizes = None if nv is None else nv.tolist()
    own, f64 = SR.own_error(words, sizes, P)
    m = got.shape[-1]
    err = (got.double().cpu() - torch.from_numpy(f64[:, :, :m, :m])).abs().amax((0, 2, 3)).numpy()
    print('spectral(permute=True) vp=%s max|dev - fp64| / yard-stick per power: %s' % (vp, ' '.join('%.2f' % (e / y) for e, y in zip(err[1:], own[1:]))))
    assert all(e <= ERR_GATE * y for e, y in zip(err[1:], own[1:])), (err, own)


# ---- 5. metrics with labels ----------------------------------------------------------------------------------------------------
def _scores(kind, rng, B, N):
    if kind == 'random':
        return (3 * rng.standard_normal((B, N, N))).astype(np.float32)
    if kind == 'ties':
        return rng.integers(0, 3, (B, N, N)).astype(np.float32)
    return np.full((B, N, N), 0.25, dtype=np.float32)


def _batch(s, sizes, N, dev):
    t = torch.from_numpy(np.ascontiguousarray(s)).clone()
    if all(n == N for n in sizes):
        return t.to(dev)
    for b, n in enumerate(sizes):
        t[b, n:, :] = 0
        t[b, :, n:] = 0
    return MaskedTensor(t.to(dev), torch.tensor(sizes, dtype=torch.int32, device=dev), (1, 2), 'N')


@pytest.mark.parametrize('kind', ['random', 'ties', 'const'])
@pytest.mark.parametrize('N', [1, 5, 64, 65, 100])
def test_metrics_with_labels_equal_the_reference_loop(N, kind):
    rng = np.random.default_rng(500 + 10 * N + len(kind))
    for sizes in ([N] * 3, [N, max(1, N // 2), max(1, N - 1)]):
        s = _scores(kind, rng, len(sizes), N)
        lab = _perms(rng, sizes, N)
        for dev in (DEV, 'cpu'):                                          # device route, host route
            x = _batch(s, sizes, N, dev)
            raw = x.tensor if isinstance(x, MaskedTensor) else x
            for fn, ref in ((accuracy_linear_assignment, R.lsap_counts), (accuracy_max, R.max_counts)):
                want = ref(raw, sizes, lab)
                assert fn(x, labels=torch.from_numpy(lab)) == (sum(want), sum(sizes)), (fn.__name__, dev)
                assert fn(x, labels=_dev(lab)) == (sum(want), sum(sizes))
                assert fn(x, aggregate_score=False, labels=torch.from_numpy(lab)) == [c / n for c, n in zip(want, sizes)]
                assert fn(x, labels=[lab[b, :n] for b, n in enumerate(sizes)]) == (sum(want), sum(sizes))
                assert fn(x) == fn(x, labels=None) == (sum(ref(raw, sizes)), sum(sizes))


def test_constant_scores_count_every_vertex_and_with_labels_the_fixed_points():
    rng = np.random.default_rng(3)
    B, N = 5, 23
    s = torch.full((B, N, N), 0.5, device=DEV)
    lab = _perms(rng, [N] * B, N)
    lab[0] = np.arange(N)
    fixed = int((lab == np.arange(N)).sum())
    assert 0 < fixed < B * N
    assert accuracy_linear_assignment(s) == (B * N, B * N)
    assert accuracy_linear_assignment(s, labels=_dev(lab)) == (fixed, B * N)
    assert accuracy_max(s, labels=_dev(lab)) == (int((lab == 0).sum()), B * N)


@pytest.mark.parametrize('name', ['rand5', 'rand64', 'ties8', 'const7', 'ragged12', 'ragged_const65'])
def test_metrics_reproduce_the_recorded_reference_outputs(name):
    g = sub(load_golden('planted_labels.npz'), name + '/')
    sizes = g['nvalid'].tolist()
    x = _batch(g['scores'].numpy(), sizes, g['scores'].shape[1], DEV)
    for fn, key in ((accuracy_linear_assignment, 'lsap'), (accuracy_max, 'max')):
        assert fn(x, labels=g['labels']) == (int(g[key + '_correct'].sum()), sum(sizes))
        assert fn(x, aggregate_score=False, labels=g['labels']) == g[key + '_acc'].tolist()


# ---- 6. all_acc_qap and greedy_qap with labels ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _decode_case(N, vp, weighted):
    """permuted pairs from the generator -> host matrices A, B (B relabelled), the unpermuted B0, device inputs, labels, scores"""
    gen = PairGenerator(N, 'ErdosRenyi', 'ErdosRenyi', edge_density=0.4, noise=0.15, vertex_proba=vp, seed=60 + N, device=DEV)
    B = 4
    b1, b2, nv = gen.bits(0, B)
    _, b2p, _, lab = gen.bits(0, B, permute=True)
    sizes = [N] * B if nv is None else nv.tolist()
    labn = lab.cpu().numpy()
    A, B0 = R.unpack_bits(b1.cpu().numpy(), N).astype(np.float64), R.unpack_bits(b2.cpu().numpy(), N).astype(np.float64)
    rng = np.random.default_rng(N)
    if weighted:                                                          # dyadic weights k / 8, not symmetric
        A, B0 = A * rng.integers(1, 8, A.shape) / 8, B0 * rng.integers(1, 8, B0.shape) / 8
    Bp = np.stack([R.relabel_matrix(B0[b], labn[b], n) for b, n in enumerate(sizes)])
    if weighted:
        x1, x2, x2p = (torch.from_numpy(m).float().to(DEV) for m in (A, B0, Bp))
        assert torch.equal(planted.relabel(x2, lab, nv), x2p)
    else:
        x1, x2, x2p = b1, b2, b2p
        assert np.array_equal(R.unpack_bits(b2p.cpu().numpy(), N), Bp.astype(np.uint8))
    s = np.zeros((B, N, N), dtype=np.float32)
    for b, n in enumerate(sizes):                                         # the planted matching as signal, plus noise
        s[b, np.arange(n), labn[b, :n]] = 2.0
        s[b, :n, :n] += (1.2 * rng.standard_normal((n, n))).astype(np.float32)
    return A, Bp, x1, x2, x2p, nv, sizes, lab, labn, torch.from_numpy(s).to(DEV)


@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('vp', [1.0, 0.7])
@pytest.mark.parametrize('N', [5, 33, 64])
def test_decoders_with_labels_equal_the_host_restatement(N, vp, weighted):
    A, Bp, x1, x2, x2p, nv, sizes, lab, labn, s = _decode_case(N, vp, weighted)
    acc, q, pl = qap.all_acc_qap(s, x1, x2p, nvalid=nv, weighted=weighted, labels=lab)
    want = R.all_acc_qap(s, A, Bp, sizes, labn)
    for got, ref in zip((acc, q, pl), want):
        assert np.array_equal(got.cpu().numpy().astype(np.float64), ref.astype(np.float64))
    # planted under labels is planted of the unpermuted pair
    assert torch.equal(pl, qap.all_acc_qap(s, x1, x2, nvalid=nv, weighted=weighted)[2])
    assert torch.equal(pl, qap.qap_objective(x1, x2p, lab, nvalid=nv, weighted=weighted)['qap'])
    # labels=None: every output equals the call without the keyword
    for a, b in zip(qap.all_acc_qap(s, x1, x2p, nvalid=nv, weighted=weighted, labels=None), qap.all_acc_qap(s, x1, x2p, nv, weighted)):
        assert torch.equal(a, b)
    start = lsap_device(s, nv, want_assign=True)[1]
    startn = start.cpu().numpy()
    for T in (0, 1, 3):
        out = qap.greedy_qap(x1, x2p, start, T, nv, weighted=weighted, labels=lab)
        for b, n in enumerate(sizes):
            s_best, acc_best, t_best = R.greedy_qap(A[b, :n, :n], Bp[b, :n, :n], startn[b, :n], T, labn[b, :n])
            assert (float(out['s_best'][b]), int(out['acc_best'][b]), int(out['T_best'][b])) == (s_best, acc_best, t_best), (T, b)
        plain, none = qap.greedy_qap(x1, x2p, start, T, nv, weighted=weighted), qap.greedy_qap(x1, x2p, start, T, nv, weighted, None)
        for k in plain:
            assert torch.equal(plain[k], none[k])
            if k != 'acc_best':
                assert torch.equal(plain[k], out[k])


# ---- 7. end to end -------------------------------------------------------------------------------------------------------------
def _ne(blocks, ragged):
    ne = dict(type='node_embedding', block_init='block_emb', block_inside='block', num_blocks=blocks, in_features=32,
              out_features=32, depth_of_mlp=3)
    if ragged:
        ne['constant_n_vertices'] = False
    return ne


@pytest.mark.parametrize('ragged', [False, True])
def test_match_on_a_relabelled_pair_is_match_on_the_pair(ragged):
    """match(x1, relabel(x2, pi), labels=pi) against match(x1, x2): planted agrees exactly; the scores are the same equivariant
    function summed in another order, S'[i][pi(j)] = S[i][j].  Bound: 2 * E2E_FWD_TOL of tests/test_gpu_parity.py on the max-norm
    relative difference, unless the fp32 CPU oracle's own difference between the two forms of this batch exceeds half of that --
    then twice the oracle's difference."""
    torch.manual_seed(31)
    B, N = 4, 20
    sizes = [9, 20, 14, 17] if ragged else [N] * B
    model = Siamese_Node_Exp(2, _ne(2, ragged)).to(DEV)
    rng = np.random.default_rng(77)
    pairs = [synthetic.make_pair(rng, n, 'ErdosRenyi', 0.3, 0.1) for n in sizes]
    l1, l2 = [torch.from_numpy(p[0]) for p in pairs], [torch.from_numpy(p[1]) for p in pairs]
    lab = _dev(_perms(rng, sizes, N))
    if ragged:
        x1, x2 = from_list(l1, (1, 2)).to(DEV), from_list(l2, (1, 2)).to(DEV)
    else:
        x1, x2 = torch.stack(l1).to(DEV), torch.stack(l2).to(DEV)
    x2p = planted.relabel(x2, lab)
    a, b = model.match(x1, x2), model.match(x1, x2p, labels=lab)
    assert torch.equal(a['planted'], b['planted'])
    assert (b['acc'] <= torch.tensor(sizes, device=DEV)).all() and (b['assign'] >= -1).all()
    sa, sb = (a['scores'].tensor, b['scores'].tensor) if ragged else (a['scores'], b['scores'])
    # the oracle in fp32 on the CPU, on both forms of the same batch
    sd = {k[len('node_embedder.'):]: v.detach().cpu() for k, v in model.state_dict().items()}
    l2p = [(x2p.tensor if ragged else x2p)[i, :, :n, :n].cpu() for i, n in enumerate(sizes)]
    o_a, o_b = O.siamese_scores_ragged(l1, l2, sd), O.siamese_scores_ragged(l1, l2p, sd)
    worst = own = 0.0
    for i, n in enumerate(sizes):
        pi = lab[i, :n].long()
        worst = max(worst, rel(sb[i, :n, :n][:, pi], sa[i, :n, :n]))
        own = max(own, rel(o_b[i][:, pi.cpu()], o_a[i]))
    tol = 2 * E2E_FWD_TOL if own <= E2E_FWD_TOL else 2 * own
    print('match on a relabelled pair, ragged=%s: scores differ by %.3g (oracle fp32 on the CPU: %.3g; bound %.3g)' % (ragged, worst, own, tol))
    assert worst < tol
