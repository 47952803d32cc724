"""ops.lbfgs_cost_grad_channels off the GPU: the sum over the channels of
reference.lbfgs_cost_grad, with a flagged pair and a table whose rows are
stored either way round."""
import numpy as np
import torch

from sagecal_amd.ops import dispatch as ops
from sagecal_amd.ops import reference as R


def test_cpu_path_is_the_sum_over_channels():
    N, T, F, nchunks, chunk_off, flagged = 5, 5, 2, [1, 2, 3], [0, 1, 3], 4
    rng = np.random.default_rng(5)
    tab = np.array([(p, q) for p in range(N) for q in range(p + 1, N)])
    tab[1::2] = tab[1::2, ::-1]
    Nbase = len(tab)

    def cplx(*shape):
        return torch.tensor(rng.standard_normal(shape)
                            + 1j * rng.standard_normal(shape))
    xs, cohs = cplx(F, T * Nbase, 2, 2), cplx(F, 3, T * Nbase, 2, 2)
    J = torch.tensor(np.eye(2)[None, None]) + 0.2 * cplx(6, N, 2, 2)
    pairs = torch.tensor(tab, dtype=torch.int32)
    pairs[flagged] = -1
    cost, grad = ops.lbfgs_cost_grad_channels(
        xs, cohs, J, ops.lbfgs_chunk_table(chunk_off, nchunks, T, 'cpu'),
        pairs, robust_nu=5.0)

    # the reference gets the flagged rows as x = coh = 0 on pair (0, 1)
    rows = torch.arange(T * Nbase) % Nbase == flagged
    xs[:, rows], cohs[:, :, rows] = 0, 0
    tab[flagged] = (0, 1)
    bb = torch.tensor(np.tile(tab, (T, 1)))
    ref = [R.lbfgs_cost_grad(xs[f], cohs[f], J, chunk_off, nchunks, bb, T,
                             Nbase, robust_nu=5.0) for f in range(F)]
    assert cost.dtype == torch.float64 and grad.shape == (6 * N * 8,)
    torch.testing.assert_close(cost, ref[0][0] + ref[1][0], rtol=1e-12,
                               atol=0)
    torch.testing.assert_close(grad, ref[0][1] + ref[1][1], rtol=0,
                               atol=1e-12 * float(grad.abs().max()))
