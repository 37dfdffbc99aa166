"""MI355X-native (gfx950) implementation of the 2-FGNN hot path of mlelarge/graph_neural_net.

Host side: the reference's nn.Module / MaskedTensor surface (``layers``, ``blocks``,
``network``, ``masked``, ``siamese``, ``losses``) and the fused ``engine``; device side:
hand-written HIP kernels in ``csrc/`` behind the C ABI of ``include/fgnn_hip.h``.
There is no CPU fallback: tensors must live on the GPU and ``libfgnn_hip.so`` must be built.
"""
__version__ = '0.1.0'
__all__ = ['WignerGenerator', 'baseline_curve']


def __getattr__(name):
    """``graph_neural_net_amd.WignerGenerator`` (wigner.py) and ``graph_neural_net_amd.baseline_curve`` (evaluation.py), imported on
    first use: importing the package stays as light as it was."""
    if name == 'WignerGenerator':
        from .wigner import WignerGenerator
        return WignerGenerator
    if name == 'baseline_curve':
        from .evaluation import baseline_curve
        return baseline_curve
    raise AttributeError('module %r has no attribute %r' % (__name__, name))
