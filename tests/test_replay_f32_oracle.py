"""The float32 restatement of the estimators (oracle/rmckf_block_f32) against the fp64 block oracle, and the teeth of the gate the GPU suite
puts on uvs_rmckf_replay_f32 with it (tests/test_gpu_replay_f32.py: E_kernel <= 2 E_f32 per case; tests/replay_f32_common.py has the
inputs and the figure).  No GPU is needed: four errors a kernel could make are injected into the restatement, by subclass and here only,
and each must exceed that gate on at least one case -- which a run of the same wrong arithmetic on the device would then do too, to within
the factor the gate already allows for a second float32 evaluation."""
import numpy as np
import pytest

import replay_f32_common as rc
from oracle import rmckf_block, rmckf_block_f32
from oracle.rmckf_block_f32 import BlockFilterF32, F32, _dot, _f32


class RowZeroRegressor(BlockFilterF32):
    """Reads dq row 0 on the first step where H = 0."""
    def _regressor(self, dq_prev):
        return dq_prev


class AnnealOneAhead(BlockFilterF32):
    """sigma of step k + 1."""
    def _sigma(self, k):
        return super()._sigma(k + 1)


class BetaIsGamma(BlockFilterF32):
    """P -= gamma g g^T in place of the Joseph form (beta = gamma (2 - gamma (a + 1)) in the kernel's rank-one statement): the two agree
    only where r = 1 and the gain is unscaled -- KF."""
    def _covariance(self, P, kk, g, h):
        return _f32(P - _f32(kk[..., :, None] * g[..., None, :]))


class HalfInnovationNorm(BlockFilterF32):
    """IMCC-KF's innovation norm over rows 0-3: the other lane's half never added."""
    def _innovation_norm(self, nu):
        return _f32(np.sqrt(_dot(nu[..., :4], nu[..., :4])))


VARIANTS = {'dq row 0 as the regressor of step 0': RowZeroRegressor, 'annealing index k + 1': AnnealOneAhead, 'covariance update with beta = gamma': BetaIsGamma,
            'IMCC-KF innovation norm over rows 0-3': HalfInnovationNorm}


@pytest.mark.parametrize('case', rc.CASES, ids=rc.case_id)
def test_float32_restatement_stays_within_2e6_of_the_fp64_oracle(case):
    out, e_f32 = rc.restatement(*case)
    ref = rc.truth(*case)
    print(f'{rc.case_id(case):44s} E_f32 {e_f32:.2e}')
    assert np.isfinite(out['X']).all()
    assert 1e-8 < e_f32 <= rc.E_F32_MAX, e_f32               # (below 1e-8 it would not be a float32 evaluation at all)
    assert np.array_equal(out['err'], (rc.inputs(*case)['f'][:, 1:] - rc.inputs(*case)['desired']))      # one float32 subtraction
    assert np.abs(out['err'] - ref['err']).max() <= 2.0 ** -24 * np.abs(ref['err']).max()


def test_float32_restatement_is_float32_throughout_and_batches_trials_independently():
    name, T, K = rc.CASES[1]
    inp = rc.inputs(name, T, K)
    filt = BlockFilterF32(inp['x0'], inp['method'], inp['kernel_bw'], inp['annealing'], inp['k_max'])
    for k in range(3):
        kappa = filt.step(inp['f'][:, k + 1] - inp['f'][:, k], inp['dq'][:, k], k)
        assert filt.X.dtype == filt.P.dtype == kappa.dtype == F32 and type(filt.sigma) is F32 and type(filt.reg) is F32
    with pytest.raises(AssertionError):
        filt.step((inp['f'][:, 4] - inp['f'][:, 3]).astype(np.float64), inp['dq'][:, 3], 3)
    whole = rc.restatement(name, T, K)[0]['X']
    alone = rmckf_block_f32.run_replay(inp['f'][7], inp['dq'][7], inp['x0'][7], inp['desired'], inp['method'], inp['kernel_bw'], inp['annealing'], inp['k_max'])
    assert alone['X'].shape == (K, 48) and np.array_equal(alone['X'], whole[7])


def test_fp64_block_oracle_is_untouched_by_the_restatement():
    """The restatement is a sibling module: the fp64 oracle keeps its double arithmetic (and, through tests/test_oracle_golden.py, its bits)."""
    filt = rmckf_block.BlockFilter(8, 6, np.ones(48, np.float32), 'GMCKF')
    filt.step(np.ones(8, np.float32), np.ones(6, np.float32), 0)
    filt.step(np.ones(8, np.float32), np.ones(6, np.float32), 1)
    assert filt.X.dtype == filt.P.dtype == np.float64


def test_injected_errors_exceed_the_gate_of_the_gpu_suite():
    """Per variant and case: E of the wrong restatement over the gate 2 E_f32(case).  Every variant must exceed it somewhere (a variant that
    does not touch a case's estimator leaves that case's bits alone: ratio 0.5)."""
    over = {}                                                # (variant, fixture) -> E_wrong / gate
    print()
    for label, cls in VARIANTS.items():
        for case in rc.CASES:
            if case[2] != rc.K_SHORT:
                continue
            gate = rc.MARGIN * rc.restatement(*case)[1]
            e_bad = rc.figure(rc.restate(*case, filter_cls=cls)['X'], *case)
            over[label, case[0]] = e_bad / gate
            print(f'{label:40s} {rc.case_id(case):44s} E_wrong {e_bad:.2e}  gate {gate:.2e}  ratio {e_bad / gate:9.1f}')
    for label in VARIANTS:
        assert max(v for (lab, _), v in over.items() if lab == label) > 1.0, (label, over)
    # and where each one must bite: row 0 everywhere, the annealing index on the sigma-30 annealed run, the covariance slip on every
    # estimator that weights (KF: beta = gamma there), the half norm on both IMCC-KF runs
    assert all(v > 1.0 for (lab, _), v in over.items() if lab == 'dq row 0 as the regressor of step 0')
    assert over['annealing index k + 1', 'closed_imcckf_sigma30_anneal'] > 1.0
    assert all(v > 1.0 for (lab, name), v in over.items() if lab == 'covariance update with beta = gamma' and '_kf_' not in name)
    assert all(v > 1.0 for (lab, name), v in over.items() if lab == 'IMCC-KF innovation norm over rows 0-3' and 'imcckf' in name)
