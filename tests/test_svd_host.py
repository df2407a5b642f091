"""CPU: the host side of the truncated SVD (rbl.RBL_svd / rbl_set_matrix_normal) — argument
validation before any GPU call, the Julia drop-in's signature, and the binding's new names."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JL = os.path.join(ROOT, "julia", "RBL_hip.jl")
HEADER = os.path.join(ROOT, "include", "rbl_hip.h")

NEW = ("rbl_set_matrix_normal", "rbl_rect_info", "rbl_get_matrix_rect", "rbl_apply_rect",
       "rbl_left_vectors")


def test_svd_argument_validation():
    """Bad arguments raise ValueError before a context is created (no GPU here)."""
    import rbl
    B = sp.random(30, 20, 0.2, format="csr", random_state=1)
    for bad in (np.zeros(5), np.zeros((2, 3, 4)), [[1.0, 2.0]], None):
        with pytest.raises(ValueError):
            rbl.RBL_svd(bad, 2, 1)
    for k in (0, -1, 21, 2.5):
        with pytest.raises(ValueError):
            rbl.RBL_svd(B, k, 1)
    with pytest.raises(ValueError):
        rbl.RBL_svd(B.T, 21, 1)
    for side in ("both", "", None):
        with pytest.raises(ValueError):
            rbl.RBL_svd(B, 2, 1, side=side)
    for b in (0, -3, 1.5):
        with pytest.raises(ValueError):
            rbl.RBL_svd(B, 2, b)


def test_julia_defines_svd_entry_point():
    src = open(JL).read()
    assert re.search(r"^function RBL_gpu_svd\(B::SparseMatrixCSC\{DOUBLE\},\s*k::Int64,\s*b::Int64\)",
                     src, re.M)
    # it uploads the SparseMatrixCSC as it is (layout 1, 1-based) and forms U on the device
    assert ":rbl_set_matrix_normal" in src and ":rbl_left_vectors" in src
    call = src[src.index(":rbl_set_matrix_normal"):]
    call = call[: call.index('"rbl_set_matrix_normal"')]
    assert re.search(r"B\.nzval,\s*Cint\(1\),\s*Cint\(1\)\)", call)


def test_new_names_in_binding_and_header():
    from rbl import _lib
    hdr = open(HEADER).read()
    for name in NEW:
        assert name in _lib.SIGNATURES, name
        assert hasattr(_lib.lib, name), name
        assert re.search(rf"^int {name}\(", hdr, re.M), name
    assert _lib.SIGNATURES["rbl_set_matrix_normal"][1][-2:] == [_lib.C.c_int, _lib.C.c_int]
    assert _lib.RBL_SPMM_KERNEL_RECT == 8 and _lib.RBL_MATRIX_FORMAT_RECT == 5
    assert re.search(r"^#define\s+RBL_SPMM_KERNEL_RECT\s+8\b", hdr, re.M)
    assert re.search(r"^#define\s+RBL_MATRIX_FORMAT_RECT\s+5\b", hdr, re.M)
    assert re.search(r"^#define\s+RBL_ABI_VERSION\s+2\b", hdr, re.M)
    import rbl
    for name in ("set_matrix_normal", "rect_info", "get_matrix_rect", "apply_rect", "left_vectors"):
        assert callable(getattr(rbl.Context, name))
    assert callable(rbl.RBL_svd)
