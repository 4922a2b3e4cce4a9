"""fbr_fourier_state_chain / Engine.fourier_state_chain against the long-double restatement of the series' Jacobian
(tests/fourier_gradient_restatement.py), entry by entry, and bit for bit against fbr_fourier_position_chain where only grad_q is given."""
import numpy as np
import pytest

import fourier_gradient_restatement as fr
from common import load_topo

pytestmark = pytest.mark.gpu
T = 7


def _cuda(a):
    import torch

    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _setup():
    from flobaroid_amd._lib import Engine

    topo = load_topo("kuka_lwr4")
    rng = np.random.default_rng(11)
    n, nh, C, R, freq = topo.num_dofs, 3, 3, 37, 10.0
    A, B = rng.standard_normal((C, n, nh)) * 0.4, rng.standard_normal((C, n, nh)) * 0.4
    wf = rng.uniform(0.8, 1.4, C)
    sample = rng.integers(-1, T, (C, R)).astype(np.int64)
    sample[0, :3] = [0, T - 1, -1]
    # rows: r % 3 == 0 one entry of grad_q only, 1 one entry of grad_dq only, 2 dense in all three (with exact zeros among them)
    g = rng.standard_normal((3, C, R, n)) * (rng.random((3, C, R, n)) < 0.7)
    kind = np.arange(R) % 3
    one = np.zeros((C, R, n))
    one[np.arange(C)[:, None], np.arange(R)[None], rng.integers(0, n, (C, R))] = 1.0
    for i in range(3):
        g[i][:, kind == 0] *= one[:, kind == 0] * (i == 0)
        g[i][:, kind == 1] *= one[:, kind == 1] * (i == 1)
    return Engine(topo, floating=False), rng, n, nh, C, R, freq, A, B, wf, sample, g


def _reference(wf, qr, A, B, sample, scale, g, freq):
    """(value, bound) per entry, (C, R, E): the chain of fourier_gradient_restatement over ONE sample per row, in long double"""
    C, R = sample.shape
    n, nh = A.shape[1:]
    E = 1 + 2 * n + 2 * n * nh
    want, bound = np.zeros((C, R, E)), np.zeros((C, R, E))
    for c in range(C):
        for r in range(R):
            if sample[c, r] < 0:
                continue
            t = np.array([np.float64(sample[c, r]) / freq])
            v, mag = fr.chain(wf[c], None if qr is None else qr[c], A[c], B[c], g[0][c, r][None], g[1][c, r][None], g[2][c, r][None], t, dtype=np.longdouble)
            sc = 1.0 if scale is None else scale[c, r]
            want[c, r] = (sc * v).astype(np.float64)
            bound[c, r] = 1e-12 * abs(sc) * mag.astype(np.float64) * (1.0 if qr is None else max(1.0, qr[c].max()))
    return want, bound


@pytest.mark.parametrize("bounded", [False, True], ids=["classic", "bounded"])
def test_state_chain_matches_the_restatement(bounded):
    """KUKA, C = 3, R = 37, three harmonics; rows with a position, a velocity or all three sensitivities, rows with sample -1; scale NULL with
    host arrays and a random scale with device tensors; one call with grad_q NULL.  Per entry |delta| <= 1e-12 |scale| sum |terms| max(1,
    q_range): the argument of test_chain_on_the_device_matches_the_restatement (tests/test_gpu_capsule_gradient.py) with the magnitude sum
    of the entry's own terms in place of sum |grad_q| -- every term is formed with a few dozen roundings of doubles, 1e-14 of its size."""
    eng, rng, n, nh, C, R, freq, A, B, wf, sample, g = _setup()
    qr = rng.uniform(0.5, 1.5, (C, n)) if bounded else None
    for scale, device in ((None, False), (rng.uniform(0.05, 1.0, (C, R)), True)):
        conv = _cuda if device else (lambda a: a)
        got = eng.fourier_state_chain(wf, A, B, conv(sample), freq, conv(g[0]), conv(g[1]), conv(g[2]), scale=conv(scale), q_range=qr)
        assert hasattr(got, "cpu") == device
        got = got.cpu().numpy() if device else got
        want, bound = _reference(wf, qr, A, B, sample, scale, g, freq)
        err = np.abs(got - want)
        print(f"bounded={bounded} device={device}: max |delta| / bound = {(err[bound > 0] / bound[bound > 0]).max():.4f}, max |entry| = {np.abs(want).max():.3f}")
        assert np.all(err <= bound), (bounded, device, float((err - bound).max()))
        assert np.abs(want).max() > 0.1
        assert np.all(got[sample < 0] == 0.0)
    # grad_q NULL: the velocity and acceleration share alone
    got = eng.fourier_state_chain(wf, A, B, sample, freq, None, g[1], g[2], q_range=qr)
    want, bound = _reference(wf, qr, A, B, sample, None, np.stack([0 * g[0], g[1], g[2]]), freq)
    assert np.all(np.abs(got - want) <= bound)
    # the same bits on every run
    assert np.array_equal(got, eng.fourier_state_chain(wf, A, B, sample, freq, None, g[1], g[2], q_range=qr))
    eng.close()


@pytest.mark.parametrize("bounded", [False, True], ids=["classic", "bounded"])
def test_position_rows_have_the_bits_of_the_position_chain(bounded):
    eng, rng, n, nh, C, R, freq, A, B, wf, sample, g = _setup()
    qr = rng.uniform(0.5, 1.5, (C, n)) if bounded else None
    scale = rng.uniform(0.05, 1.0, (C, R))
    for sc in (None, scale):
        pos = eng.fourier_position_chain(wf, A, B, sample, g[0], freq, scale=sc, q_range=qr)
        assert np.array_equal(eng.fourier_state_chain(wf, A, B, sample, freq, g[0], scale=sc, q_range=qr), pos)
        dev = eng.fourier_state_chain(wf, A, B, _cuda(sample), freq, _cuda(g[0]), scale=_cuda(sc), q_range=qr)
        assert np.array_equal(dev.cpu().numpy(), pos)
    assert np.abs(pos).max() > 0.1
    eng.close()


def test_bad_arguments_are_refused():
    from flobaroid_amd._lib import FbrError

    eng, rng, n, nh, C, R, freq, A, B, wf, sample, g = _setup()
    with pytest.raises(FbrError, match="code -1"):
        eng.fourier_state_chain(wf, A, B, sample, 0.0, g[0], g[1], g[2])  # freq must be positive
    with pytest.raises(ValueError):
        eng.fourier_state_chain(wf, A, B, sample, freq)  # no sensitivities at all
    eng.close()
