"""rbl — MI355X-native Randomized Block Lanczos inner loop (host side).

``RBL_gpu(A, k, b)`` mirrors Julia/RBL_gpu.jl:205, ``RBL_thick(A, k, b, max_blocks=m)`` the same
eigenpairs by thick-restart block Lanczos in a basis bounded by m + 1 blocks (``lanczos_thick`` on a
loaded context; ``RBL_svd(..., max_blocks=m)`` for singular triplets), ``RBL_svd(B, k, b)`` the truncated SVD of
images.jl:20-33 on the implicit B^T B (``shift=(u, v)``: of B - u v^T), ``RBL_pca(B, k, b)`` PCA of a
sparse B with implicit centring on top of it, ``RBL_filtered(A, k, b, which="SA"|"LA")`` the smallest or
largest eigenpairs through a Chebyshev filter, ``RBL_interior(A, k, b, sigma)`` the eigenpairs
nearest sigma through a Chebyshev delta series, ``RBL_interval(A, (x0, x1), b)`` all eigenpairs in
an interval (``spectral_density`` / ``eig_count``: the Chebyshev moments behind it); each of the
square-A drivers takes ``update=(P, S)`` for the implicit operator A + P S P^T (``rbl.lowrank``:
``modularity_update``, ``deflation_update``, ``centering_update``, ``RBL_modularity``);
``apply_function`` / ``trace_function`` / ``diag_function`` (``rbl.funm``) give f(A) B, tr f(A) and
diag f(A) by Chebyshev series (``heat_kernel_signature``, ``subgraph_centrality``, ``local_density``,
``logdet``); a ``KernelMatrix(X, kind, gamma)`` (``rbl.kernelop``) is the implicit kernel matrix over
the rows of X as the A of any of these (``RBL_kernel_pca``, ``RBL_spectral_embedding``,
``kernel_centering_update``), and ``kernel_pca_fit`` / ``spectral_embedding_fit`` / ``gp_fit`` keep such a
fit as a model that serves points outside the training set (``transform``, ``predict``) through the
cross-kernel product ``Context.kernel_cross``; ``kernel_gradients`` and ``GPModel.mll_gradient`` give
hyperparameter gradients through the derivative product ``Context.kernel_hadamard``; ``knn_graph(X, m)``
(``rbl.knn``: ``knn_lists``, ``graph_from_knn``) builds the m-nearest-neighbour graph of the points on the
device (``Context.kernel_knn``) as a sparse A, and ``RBL_spectral_embedding`` / ``spectral_embedding_fit`` take
``neighbors=m`` to run on it; ``kmeans(X, c)`` (``rbl.kmeans``) is Lloyd's iteration with k-means++
seeding on the device, and ``RBL_spectral_clustering`` / ``spectral_clustering_fit`` run it on the
embedding and return labels; ``solve(A, B, shift=)`` (``rbl.solve``) solves
(A + shift I) X = B on any of these operators by batched preconditioned CG
(``spectral_preconditioner``, ``cg_tridiag``, ``logdet_lanczos``); ``pivoted_cholesky(K, r)``
(``rbl.pchol``) is the partial pivoted Cholesky factor of a kernel matrix on the device
(``Context.kernel_pchol``), and ``pchol_preconditioner`` turns it into a CG preconditioner without an
eigensolve (``gp_fit(..., precond="pchol")``); ``Context`` wraps the C-ABI of
librbl_hip.so (include/rbl_hip.h).  Importing this package loads the HIP library and fails
loudly if it has not been built: there is no CPU fallback.
"""
from ._lib import RBLError, lib, stage_names  # noqa: F401  (raises ImportError if unbuilt)
from .host import TBand, check_convergence, dsbev, sort_eig_abs  # noqa: F401
from . import io  # noqa: F401
from .restarted import RBL_gpu_restarted, RBL_restarted  # noqa: F401
from .rbl_gpu import (KRYL_SZ_GPU, RESIDUAL_TOL, Context, RBL_gpu, RBLInfo, LocalGroup,  # noqa: F401
                      lanczos, rccl_version)
from .svd import RBL_svd  # noqa: F401
from .thick import RBL_thick, lanczos_thick, projected_matrix  # noqa: F401
from .pca import PCAResult, RBL_pca, column_stats  # noqa: F401
from .filtered import RBL_filtered, cheb_scalars, filter_bounds, lanczos_filtered  # noqa: F401
from .interior import (RBL_interior, delta_coeffs, estimate_spectrum, lanczos_interior,  # noqa: F401
                       series_eval, spectrum_bounds)
from .density import (RBL_interval, check_moments, eig_count, interval_degree, interval_run,  # noqa: F401
                      jackson, kpm_count, kpm_density, spectral_density)
from .lowrank import (RBL_modularity, centering_update, deflation_update,  # noqa: F401
                      modularity_update)
from .kernelop import (GPModel, KernelGradient, KernelMatrix, KernelPCAModel, MLLGradient,  # noqa: F401
                       RBL_kernel_pca, RBL_spectral_embedding, SpectralEmbeddingModel, cross_splits, gp_fit,
                       hadamard_max_rank, kernel_centering_update, kernel_gradients, kernel_pca_fit,
                       row_normalize, scale_gradient_sums, spectral_embedding_fit)
from .knn import (KnnSpectralEmbeddingModel, graph_from_knn, knn_graph, knn_lists,  # noqa: F401
                  knn_nystrom_algebra, knn_weights, normalized_affinity)
from .kmeans import (KMeansResult, RBL_spectral_clustering, SpectralClusteringModel, kmeans,  # noqa: F401
                     kmeans_predict, seeding_uniforms, select_best, spectral_clustering_fit)
from .funm import (DiagResult, apply_function, cheb_coeffs, cheb_fit, diag_function, diag_series,  # noqa: F401
                   heat_kernel_signature, local_density, logdet, subgraph_centrality, trace_function)
from .solve import (SolveInfo, cg_tridiag, lanczos_quadrature, logdet_lanczos, solve,  # noqa: F401
                    spectral_preconditioner)
from .pchol import (PivotedCholesky, pchol_eigenpairs, pchol_preconditioner, pivoted_cholesky,  # noqa: F401
                    precond_logdet_terms)
