"""The PCA fit of the HIP path (vsc_hip/pca_fit.py), stated in numpy float64 -- the yardstick of tests/test_pca_fit_cpu.py and
tests/test_gpu_pca_fit.py; the code under test never is.

Two-pass covariance with the n - 1 divisor, ``numpy.linalg.eigh``, eigenvalues descending, and sklearn 1.7's sign rule
(``svd_flip(u_based_decision=False)``): the coordinate of largest magnitude of every component is positive, the first such
index on a tie.  ``explained_variance_`` = eigenvalues, no whitening.  Equals ``PCA(svd_solver="full")`` on float64 input."""
from types import SimpleNamespace

import numpy as np


def covariance(x):
    x = np.asarray(x, dtype=np.float64)
    mean = x.mean(axis=0)
    c = x - mean
    return mean, c.T @ c / (len(x) - 1)


def fit(x, n_components):
    mean, cov = covariance(x)
    w, v = np.linalg.eigh(cov)
    order = np.argsort(w, kind="stable")[::-1][:n_components]
    comps = v[:, order].T
    lead = np.argmax(np.abs(comps), axis=1)
    comps = comps * np.where(comps[np.arange(len(comps)), lead] < 0, -1.0, 1.0)[:, None]
    return SimpleNamespace(mean_=mean, components_=comps, explained_variance_=w[order], whiten=False, n_components_=n_components,
                           n_samples_=len(x))


def transform(model, x):
    return (np.asarray(x, dtype=np.float64) - model.mean_) @ model.components_.T


def spectrum_data(seed, n, d, ratio, offset=0.0):
    """[n, d] float32 with a geometric spectrum: bell-shaped noise (tools/synth.py) scaled by ratio^j along the axes of a fixed
    orthogonal basis, plus a common offset."""
    import sys, os
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from tools import synth
    z = synth.normalish(seed, (n, d)).astype(np.float64) * ratio ** np.arange(d)
    q, _ = np.linalg.qr(synth.normalish(seed + 1, (d, d)).astype(np.float64))
    return (z @ q.T + offset).astype(np.float32)
