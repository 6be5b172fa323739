"""PCA fit on the HIP path (reference: infer/concat_pca_sn.py:42-54, ``PCA(n_components, random_state=2023).fit``).

``HipPCAFit(d)`` accumulates the raw moments sum x and sum x x^T of fp32 rows on the device in fp64 (vsc_pca_fit_* in
include/vsc_hip.h, csrc/pca_fit.hip); ``finalize(k)`` copies the d x d covariance to the host and solves the eigenproblem
there with ``numpy.linalg.eigh`` in float64 -- that step does not depend on the number of rows (0.8 s at d = 2048).

The contract (tests/pca_contract.py states it in numpy): float64 covariance with the n - 1 divisor, eigh, eigenvalues
descending, and sklearn 1.7's sign rule -- ``svd_flip(u_based_decision=False)``: the coordinate of largest magnitude of every
component is positive, ties going to the lowest index; ``explained_variance_`` = eigenvalues, ``whiten = False``.  This is
sklearn's ``svd_solver="full"`` on float64 input; the reference's default picks the randomized solver for its shapes and is
approximate.

No sklearn, no pickle: the fitted model is a plain object that ``src.query_postprocess.HipPCA`` takes as it is and
``save_pca_model`` writes as an .npz.
"""
from __future__ import annotations

import ctypes

import numpy as np

MIN_D, MAX_D = 16, 4096      # limits of the kernel (include/vsc_hip.h, vsc_pca_fit_create)


class FittedPCA:
    """What ``HipPCA`` reads of sklearn's fitted ``PCA``: ``mean_`` [d] and ``components_`` [k, d] float32 (the dtype HipPCA
    computes in), ``explained_variance_`` [k] float64, ``whiten``, ``n_components_``, ``n_samples_``."""

    FIELDS = ("mean_", "components_", "explained_variance_", "whiten", "n_components_", "n_samples_")

    def __init__(self, mean_, components_, explained_variance_, whiten=False, n_components_=None, n_samples_=0):
        self.mean_ = np.ascontiguousarray(mean_, dtype=np.float32)
        self.components_ = np.ascontiguousarray(components_, dtype=np.float32)
        self.explained_variance_ = np.ascontiguousarray(explained_variance_, dtype=np.float64)
        self.whiten = bool(whiten)
        self.n_components_ = int(len(self.components_) if n_components_ is None else n_components_)
        self.n_samples_ = int(n_samples_)


def components_from_covariance(cov: np.ndarray, n_components: int):
    """float64 symmetric [d, d] -> (components [k, d], eigenvalues [k]) by the contract: eigh, descending, each component's
    coordinate of largest magnitude positive (first such index on a tie)."""
    w, v = np.linalg.eigh(np.asarray(cov, dtype=np.float64))
    order = np.argsort(w, kind="stable")[::-1][:n_components]
    w, comps = w[order], v[:, order].T
    lead = np.argmax(np.abs(comps), axis=1)
    signs = np.sign(comps[np.arange(len(comps)), lead])
    signs[signs == 0] = 1.0
    return comps * signs[:, None], w


class HipPCAFit:
    """Streaming fit: ``partial_fit`` any number of [n, d] fp32 blocks, then ``finalize(n_components)``."""

    def __init__(self, d: int):
        from vsc_hip import _lib
        if not MIN_D <= int(d) <= MAX_D:
            raise ValueError(f"{d} features outside the kernel's [{MIN_D}, {MAX_D}]")
        self._lib = _lib.require_device()
        self.d = int(d)
        handle = ctypes.c_void_p()
        _lib.check(self._lib.vsc_pca_fit_create(self.d, ctypes.byref(handle)))
        self._h = handle

    def close(self):
        if getattr(self, "_h", None):
            self._lib.vsc_pca_fit_destroy(self._h)
            self._h = None

    __del__ = close

    def partial_fit(self, x):
        """x: numpy array or device tensor, fp32, [n, d] (rows may be strided: a column slice of a wider matrix)."""
        import torch

        from vsc_hip import _lib
        if isinstance(x, np.ndarray):
            x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
        if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.shape[1] == self.d):
            raise ValueError(f"partial_fit takes fp32 [n, {self.d}] on the device, not {x.dtype} {tuple(x.shape)} on {x.device}")
        if x.shape[0] == 0:
            return self
        if x.stride(1) != 1 or (x.shape[0] > 1 and x.stride(0) < self.d):
            x = x.contiguous()
        ld = x.stride(0) if x.shape[0] > 1 else self.d
        _lib.check(self._lib.vsc_pca_fit_update_f32(self._h, ctypes.c_void_p(x.data_ptr()), x.shape[0], ld, _lib.current_stream()))
        torch.cuda.current_stream().synchronize()      # x may be a temporary of this call
        return self

    @property
    def n_samples(self) -> int:
        from vsc_hip import _lib
        n = ctypes.c_int64()
        _lib.check(self._lib.vsc_pca_fit_moments_f64(self._h, None, None, ctypes.byref(n), None))
        return int(n.value)

    def moments(self):
        """-> (sum [d], S2 [d, d]) float64 device tensors; S2 is the full symmetric matrix."""
        import torch

        from vsc_hip import _lib
        s = torch.empty(self.d, dtype=torch.float64, device="cuda")
        s2 = torch.empty((self.d, self.d), dtype=torch.float64, device="cuda")
        _lib.check(self._lib.vsc_pca_fit_moments_f64(self._h, _lib.ptr(s), _lib.ptr(s2), None, _lib.current_stream()))
        return s, s2

    def covariance(self):
        """-> (mean [d], covariance [d, d] with the n - 1 divisor) float64 device tensors; needs two rows."""
        import torch

        from vsc_hip import _lib
        mean = torch.empty(self.d, dtype=torch.float64, device="cuda")
        cov = torch.empty((self.d, self.d), dtype=torch.float64, device="cuda")
        _lib.check(self._lib.vsc_pca_fit_covariance_f64(self._h, _lib.ptr(mean), _lib.ptr(cov), _lib.current_stream()))
        return mean, cov

    def finalize(self, n_components: int) -> FittedPCA:
        n = self.n_samples
        if not 1 <= n_components <= self.d:
            raise ValueError(f"n_components {n_components} outside [1, {self.d}]")
        if n <= n_components:
            raise ValueError(f"{n} rows seen: a fit of {n_components} components needs more rows than components")
        mean, cov = self.covariance()
        comps, var = components_from_covariance(cov.cpu().numpy(), n_components)
        return FittedPCA(mean.cpu().numpy(), comps, var, whiten=False, n_components_=n_components, n_samples_=n)
