"""The reference's observability analysis of a trajectory (trajectory.py:226-264) restated on a materialised ``YBase`` with
``numpy.linalg.svd``: singular values below ``threshold`` times the largest are unobservable; the squared components of their right
singular vectors, summed per base parameter, are carried to the identified parameters by ``Pb`` (base parameter j is identified parameter
``independent_cols[j]``), and every identified parameter with a score above 0.5 is listed."""
import numpy as np


def observability(YBase, independent_cols, num_identified, threshold=1e-6):
    """dict with the three keys of the trajectory file (``unobservable_params`` int64, ``observability_threshold``,
    ``n_observable_base_params``) and, for the tests, ``energy`` (nb,), ``score`` (num_identified,) and the singular values ``S``"""
    cols = np.asarray(independent_cols, dtype=np.int64)
    nb = YBase.shape[1]
    assert cols.shape == (nb,)
    S, Vt = np.linalg.svd(YBase, full_matrices=False)[1:]
    n_unobs = int(np.sum(S < S[0] * threshold))
    energy = np.zeros(nb)
    if n_unobs > 0:
        energy = np.sum(Vt[-n_unobs:, :] ** 2, axis=0)
    Pb = np.zeros((int(num_identified), nb))
    Pb[cols, np.arange(nb)] = 1.0
    score = Pb @ energy
    idx = np.where(score > 0.5)[0].tolist() if n_unobs > 0 else []
    return {"unobservable_params": np.array(idx, dtype=np.int64), "observability_threshold": threshold, "n_observable_base_params": nb - n_unobs,
            "energy": energy, "score": score, "S": S}
