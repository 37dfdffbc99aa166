"""Price of the decode chain on real-weighted pairs (evaluation.decode_scores_weighted; csrc/qap_2opt_weighted.hip,
csrc/qap_fold_weighted.hip): 32 spectral pairs (PairGenerator.spectral: Regular parents with ErdosRenyi noise 0.1, channel 0 = L =
D^-1/2 W D^-1/2, read in place out of the 4-channel batch) at N = 50 (A and Bp in LDS) and N = 200 (Bp in the workspace), 8 revealed
seeds per pair (rows 0, N/8, 2 N/8, .. fixed to themselves: the pairs are not relabelled).  The scores are 2 I + standard normal
noise from the device's generator: an informative start that leaves the later stages work to do.  The exchange searches start from
the matching of the seeded FAQ stage, which is a permutation that holds every seed, so both instantiations run from the same start.

(a) the fgnn_qapw_2opt_seeded launch (8 seeds; and with seeds of all -1, the same scan as without) against the fgnn_qapw_2opt launch;
(b) the fgnn_qapw_fold launch against the torch composition that forms the same sums from the same per-pair tensors;
(c) decode_scores_weighted per stage: the chain with no stage, with faq, with faq and two_opt, with refine = 2, with seeds, faq and
    two_opt; the differences are the stages' prices;
(d) the unseeded fgnn_qapw_2opt of this build against the parent commit's library (--parent-lib, the same Python driving both):
    the template parameter is meant to leave that path alone, so the difference should sit within the windows' spread.

Protocol (tools/time_pairgen_indexed.py): device events on one stream, warm-up, then WINDOWS = 7 rounds in which the variants take
turns with one window of `reps` calls each; reported per variant: the median window and the spread of the same run.  One timed probe
of the unseeded launch first: `reps` is cut so that its windows stay within --budget seconds.
usage: python tools/time_decode_weighted.py [--reps 20] [--sizes 50,200] [--budget 20] [--parent-lib lib.so]
                                            [--out profiles/decode_weighted_time.json]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from graph_neural_net_amd import _lib, qap
from graph_neural_net_amd.evaluation import WeightedQapMeter, decode_scores_weighted
from graph_neural_net_amd.pairgen import PairGenerator
from time_pairgen_indexed import DEV, WINDOWS, alternate, row, window
from time_restarts import load_parent

B = 32
SEEDS = 8


def torch_fold(assign, perm, q, planted, refined, target):
    """the sums of fgnn_qapw_fold from the same per-pair tensors, composed in torch (full corners, identity targets) -> 14 values"""
    N = assign.shape[1]
    hit, rhit = (assign == target).sum(1), (perm == target).sum(1)
    matched = ((assign >= 0) & (assign < N)).all(1)
    has = matched & (planted > 0)
    ratio = torch.where(has, q.double() / planted.double(), torch.zeros_like(q, dtype=torch.float64))
    m = matched.double()
    return torch.stack([ratio.sum(), (q.double() * m).sum(), (planted.double() * m).sum(), (refined.double() * m).sum(),
                        has.sum().double(), hit.sum().double(), (rhit * matched).sum().double(), (matched & (q >= planted)).sum().double(),
                        (matched & (hit == N)).sum().double(), (matched & (refined > q)).sum().double(), (~matched).sum().double()])


def one_size(N, reps, budget, parent):
    gen = PairGenerator(N, 'Regular', 'ErdosRenyi', noise=0.1, seed=1, device=DEV)
    f1, f2 = (d['input'] for d in gen.spectral(0, B))
    g = torch.Generator(device=DEV).manual_seed(N)
    s = torch.randn(B, N, N, generator=g, device=DEV) + 2 * torch.eye(N, device=DEV)
    seeds = torch.full((B, N), -1, dtype=torch.int32, device=DEV)
    rows = torch.arange(0, N, max(N // SEEDS, 1), device=DEV)[:SEEDS]
    seeds[:, rows] = rows.to(torch.int32)
    free = torch.full((B, N), -1, dtype=torch.int32, device=DEV)
    target = torch.arange(N, dtype=torch.int32, device=DEV).expand(B, N).contiguous()
    # the start of the searches and the tensors of the fold: one seeded chain, read before the timing
    out = decode_scores_weighted(s, f1, f2, two_opt=True, faq=True, seeds=seeds)
    start = torch.where((out['faq_status'] == 2)[:, None], out['assign'], out['faq_perm']).contiguous()
    assign, perm, q, planted, refined = (out[k].contiguous() for k in ('assign', 'perm', 'qap', 'planted', 'refined'))
    quality = {'qap_ratio': float((q.double() / planted.double()).mean()),
               'refined_qap_ratio': float((refined.double() / planted.double()).mean()), 'swaps_mean': float(out['swaps'].double().mean()),
               'status': sorted(set(out['status'].cpu().tolist())), 'faq_status': sorted(set(out['faq_status'].cpu().tolist()))}
    x1, x2, gs, ld = qap.weighted_views(f1, f2)
    nbytes = _lib.load().fgnn_qapw_2opt_ws_bytes(B, N)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV) if nbytes else None
    po = torch.empty(B, N, dtype=torch.int32, device=DEV)
    o32 = torch.empty(2, B, dtype=torch.int32, device=DEV)
    nit = torch.empty(B, dtype=torch.int64, device=DEV)
    tail = (B, N, -1, _lib.ptr(ws), nbytes, _lib.ptr(po), _lib.ptr(o32[0]), _lib.ptr(nit), _lib.ptr(o32[1]))

    def launch():
        _lib.call('fgnn_qapw_2opt', _lib.ptr(x1), _lib.ptr(x2), gs, ld, _lib.ptr(start), None, *tail, _lib.stream_ptr())

    def launch_seeded(sd):
        return lambda: _lib.call('fgnn_qapw_2opt_seeded', _lib.ptr(x1), _lib.ptr(x2), gs, ld, _lib.ptr(start), _lib.ptr(sd), None, *tail,
                                 _lib.stream_ptr())

    def launch_parent():
        rc = parent.fgnn_qapw_2opt(_lib.ptr(x1), _lib.ptr(x2), gs, ld, _lib.ptr(start), None, *tail, _lib.stream_ptr())
        if rc != 0:
            raise RuntimeError('the parent library refused fgnn_qapw_2opt')
    meter = WeightedQapMeter(DEV)

    def fold():
        _lib.call('fgnn_qapw_fold', _lib.ptr(assign), _lib.ptr(perm), None, _lib.ptr(q), _lib.ptr(planted), _lib.ptr(refined), None, B, N,
                  B, None, None, None, _lib.ptr(meter.buf), _lib.stream_ptr())
    launch()
    torch.cuda.synchronize()
    probe = window(launch, 1)
    reps = max(1, min(reps, int(budget * 1e6 / (WINDOWS * probe))))
    searches = {'two_opt_launch': launch, 'two_opt_seeded_launch': launch_seeded(seeds), 'two_opt_seeded_all_free_launch': launch_seeded(free)}
    if parent is not None:
        searches['two_opt_launch_parent_lib'] = launch_parent
    t = alternate(searches, reps)
    tf = alternate({'fold_launch': fold, 'fold_torch': lambda: torch_fold(assign, perm, q, planted, refined, target)}, max(reps, 20))
    chain = {'chain_plain': dict(), 'chain_faq': dict(faq=True), 'chain_faq_two_opt': dict(faq=True, two_opt=True),
             'chain_refine2': dict(refine=2), 'chain_seeds_faq_two_opt': dict(faq=True, two_opt=True, seeds=seeds)}
    tc = alternate({k: (lambda kw=kw: decode_scores_weighted(s, f1, f2, meter=meter, **kw)) for k, kw in chain.items()}, max(1, reps // 4))
    res = {'n_vertices': N, 'pairs': B, 'seeds_per_pair': SEEDS, 'reps': reps, 'probe_us': round(probe, 2), 'search': row(t),
           'seeded_minus_unseeded_us': round(t['two_opt_seeded_launch'][0] - t['two_opt_launch'][0], 2),
           'all_free_minus_unseeded_us': round(t['two_opt_seeded_all_free_launch'][0] - t['two_opt_launch'][0], 2),
           'fold': row(tf), 'fold_over_torch': round(tf['fold_launch'][0] / tf['fold_torch'][0], 3), 'chain': row(tc),
           'stage_us': {'faq': round(tc['chain_faq'][0] - tc['chain_plain'][0], 2),
                        'two_opt_after_faq': round(tc['chain_faq_two_opt'][0] - tc['chain_faq'][0], 2),
                        'refine2': round(tc['chain_refine2'][0] - tc['chain_plain'][0], 2),
                        'seeds_on_faq_two_opt': round(tc['chain_seeds_faq_two_opt'][0] - tc['chain_faq_two_opt'][0], 2)},
           'quality': quality}
    if parent is not None:
        res['unseeded_minus_parent_us'] = round(t['two_opt_launch'][0] - t['two_opt_launch_parent_lib'][0], 2)
        res['unseeded_spread_us'] = round(max(t[k][2] - t[k][1] for k in ('two_opt_launch', 'two_opt_launch_parent_lib')), 2)
    for name, tt in (('search', t), ('fold', tf), ('chain', tc)):
        print('N %d %s  ' % (N, name) + '  '.join('%s %.2f us (%.2f - %.2f)' % ((k,) + tt[k]) for k in tt), flush=True)
    print('N %d  quality %s' % (N, json.dumps(quality)), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--sizes', default='50,200')
    ap.add_argument('--budget', type=float, default=20.0)
    ap.add_argument('--parent-lib', default=None)
    ap.add_argument('--out', default=None)
    o = ap.parse_args()
    _lib.load()
    parent = load_parent(o.parent_lib) if o.parent_lib else None
    res = {'tool': 'time_decode_weighted', 'windows': WINDOWS, 'parent_lib': bool(parent), 'sizes': []}
    for n in map(int, o.sizes.split(',')):          # (the file is rewritten after every size: a long run leaves what it finished)
        res['sizes'].append(one_size(n, o.reps, o.budget, parent))
        line = json.dumps(res)
        if o.out:
            os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
            with open(o.out, 'w') as f:
                f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
