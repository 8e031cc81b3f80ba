"""In-house classical AMG setup (amg_classical_*): the hierarchy the reference
gets from HYPRE_BoomerAMGSetup (SMEM_Setup.cpp:55-70, DMEM_Setup.cpp:169-173),
built by the library -- strength of connection, HMIS / PMIS coarsening,
extended+i or direct interpolation, optional truncation of P (P_max_elmts /
trunc_factor), Galerkin R A P, and the explicit smoothed transfers of MULTADD
(smooth_transfers, optionally truncated).  On the host by default; device=d moves
the products and the truncation to that GPU, setup_on_device=1 the whole level
loop (HMIS still coarsens on the host), bit-identical either way.  strength,
transpose, pmis and interp run one phase on its own, on the host or a GPU."""
import ctypes as C

import numpy as np

from . import abi
from .abi import (AMG_CLASSICAL_DIRECT, AMG_CLASSICAL_EXT_I, AMG_COARSEN_HMIS,  # noqa: F401
                  AMG_COARSEN_PMIS, AMG_COARSEN_PMIS_FIXED, AMG_GEN_A, AMG_GEN_P, AMG_GEN_PS, AMG_GEN_R,
                  AMG_GEN_RS)


def elasticity(refine):
    """The DMEM elasticity problem (amg_elast_*): (n, rowptr, col, val, rhs) as
    numpy copies; num_functions = 3 (byVDIM)."""
    from . import check, lib
    h = C.c_void_p()
    check(lib.amg_elast_create(int(refine), C.byref(h)))
    try:
        n, nz = C.c_int(), C.c_longlong()
        rp, cj, v, b = abi._ip(), abi._ip(), abi._dp(), abi._dp()
        check(lib.amg_elast_get(h, C.byref(n), C.byref(nz), C.byref(rp), C.byref(cj), C.byref(v), C.byref(b)))
        N, Z = n.value, nz.value
        return (N, np.ctypeslib.as_array(rp, (N + 1,)).copy(), np.ctypeslib.as_array(cj, (Z,)).copy(),
                np.ctypeslib.as_array(v, (Z,)).copy(), np.ctypeslib.as_array(b, (N,)).copy())
    finally:
        lib.amg_elast_free(h)


def default_opts(**kw):
    """SMEM parameters (SMEM_Main.cpp:29-35): HMIS, ext+i, theta 0.25; DMEM uses
    coarsen_type=9, strong_threshold=0.5 (DMEM_Main.cpp:38-49)."""
    from . import lib
    o = abi.AmgClassicalOpts()
    lib.amg_classical_opts_default(C.byref(o))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise AttributeError(k)
        setattr(o, k, v)
    return o


def truncate_rows(n, rowptr, col, val, trunc_factor, max_elmts, device=-1):
    """amg_csr_truncate: the rows of a CSR truncated by the interpolation
    truncation rule (include/amg_mi355x.h), on the host (device -1) or on that
    GPU; numpy (rowptr, col, val)."""
    from . import check, lib
    rp = np.ascontiguousarray(rowptr, dtype=np.int32)
    cj = np.ascontiguousarray(col, dtype=np.int32)
    v = np.ascontiguousarray(val, dtype=np.float64)
    orp = np.zeros(int(n) + 1, dtype=np.int32)
    ocj = np.zeros(max(cj.size, 1), dtype=np.int32)
    ov = np.zeros(max(v.size, 1), dtype=np.float64)
    nz = C.c_longlong()
    check(lib.amg_csr_truncate(int(device), int(n), rp.ctypes.data_as(abi._ip), cj.ctypes.data_as(abi._ip),
                               v.ctypes.data_as(abi._dp), float(trunc_factor), int(max_elmts),
                               orp.ctypes.data_as(abi._ip), ocj.ctypes.data_as(abi._ip), ov.ctypes.data_as(abi._dp),
                               C.byref(nz)))
    return orp, ocj[:nz.value].copy(), ov[:nz.value].copy()


def spgemm(A, B, device=-1):
    """amg_csr_spgemm: C = A B by the setup's rule (Gustavson order, sorted
    columns, diagonal first when C is square), on the host (device -1) or on
    that GPU; A, B and C are (nrows, ncols, rowptr, col, val) like
    ClassicalAMG.get."""
    from . import check, lib
    an, am, arp, acj, av = A
    bn, bm, brp, bcj, bv = B
    if int(am) != int(bn):
        raise ValueError(f"spgemm: A has {am} columns, B has {bn} rows")
    arp, brp = (np.ascontiguousarray(x, dtype=np.int32) for x in (arp, brp))
    acj, bcj = (np.ascontiguousarray(x, dtype=np.int32) for x in (acj, bcj))
    av, bv = (np.ascontiguousarray(x, dtype=np.float64) for x in (av, bv))
    if arp.size != int(an) + 1 or brp.size != int(bn) + 1:
        raise ValueError("spgemm: rowptr length")
    if acj.size != av.size or bcj.size != bv.size or acj.size < arp[-1] or bcj.size < brp[-1]:
        raise ValueError("spgemm: col / val length")
    h = abi.AmgHostCsr()
    check(lib.amg_csr_spgemm(int(device), int(an), int(am), arp.ctypes.data_as(abi._ip),
                             acj.ctypes.data_as(abi._ip), av.ctypes.data_as(abi._dp), int(bm),
                             brp.ctypes.data_as(abi._ip), bcj.ctypes.data_as(abi._ip), bv.ctypes.data_as(abi._dp),
                             C.byref(h)))
    try:
        n, z = h.nrows, h.nnz
        return (n, h.ncols, np.ctypeslib.as_array(h.rowptr, (n + 1,)).copy(),
                np.ctypeslib.as_array(h.col, (z,)).copy() if z else np.zeros(0, np.int32),
                np.ctypeslib.as_array(h.val, (z,)).copy() if z else np.zeros(0))
    finally:
        lib.amg_host_csr_free(C.byref(h))


def set_spgemm_scratch(slots):
    """amg_set_spgemm_scratch: the device product's scratch budget in table
    slots per batch of rows, process-wide; 0 restores the default."""
    from . import check, lib
    check(lib.amg_set_spgemm_scratch(int(slots)))


def _host_csr(h, values=True):
    """(nrows, ncols, rowptr, col, val) numpy copies of an AmgHostCsr, then freed"""
    from . import lib
    try:
        n, z = h.nrows, h.nnz
        return (n, h.ncols, np.ctypeslib.as_array(h.rowptr, (n + 1,)).copy(),
                np.ctypeslib.as_array(h.col, (z,)).copy() if z else np.zeros(0, np.int32),
                (np.ctypeslib.as_array(h.val, (z,)).copy() if z else np.zeros(0)) if values else None)
    finally:
        lib.amg_host_csr_free(C.byref(h))


def _csr_args(rowptr, col, val=None):
    rp = np.ascontiguousarray(rowptr, dtype=np.int32)
    cj = np.ascontiguousarray(col, dtype=np.int32)
    v = None if val is None else np.ascontiguousarray(val, dtype=np.float64)
    if rp.size < 1 or cj.size < rp[-1] or (v is not None and v.size < rp[-1]):
        raise ValueError("rowptr / col / val length")
    return rp, cj, v


def strength(n, rowptr, col, val, theta, max_row_sum=1.0, num_functions=1, device=-1):
    """amg_csr_strength: the strength pattern S of a square CSR, (rowptr, col),
    on the host (device -1) or on that GPU."""
    from . import check, lib
    rp, cj, v = _csr_args(rowptr, col, val)
    if rp.size != int(n) + 1:
        raise ValueError("strength: rowptr length")
    h = abi.AmgHostCsr()
    check(lib.amg_csr_strength(int(device), int(n), rp.ctypes.data_as(abi._ip), cj.ctypes.data_as(abi._ip),
                               v.ctypes.data_as(abi._dp), float(theta), float(max_row_sum), int(num_functions),
                               C.byref(h)))
    return _host_csr(h, values=False)[2:4]


def transpose(n, m, rowptr, col, val=None, device=-1):
    """amg_csr_transpose: the transpose of an n x m CSR by the setup's rule,
    (rowptr, col, val); val None: the pattern alone, (rowptr, col, None)."""
    from . import check, lib
    rp, cj, v = _csr_args(rowptr, col, val)
    if rp.size != int(n) + 1:
        raise ValueError("transpose: rowptr length")
    h = abi.AmgHostCsr()
    check(lib.amg_csr_transpose(int(device), int(n), int(m), rp.ctypes.data_as(abi._ip), cj.ctypes.data_as(abi._ip),
                                None if v is None else v.ctypes.data_as(abi._dp), C.byref(h)))
    return _host_csr(h, values=v is not None)[2:]


def pmis(n, s_rowptr, s_col, seed, device=-1):
    """amg_cf_pmis: the PMIS marker (1 = C, -1 = F) of a strength pattern; seed
    is the per-level seed (include/amg_mi355x.h)."""
    from . import check, lib
    rp, cj, _ = _csr_args(s_rowptr, s_col)
    if rp.size != int(n) + 1:
        raise ValueError("pmis: rowptr length")
    cf = np.zeros(int(n), dtype=np.int32)
    check(lib.amg_cf_pmis(int(device), int(n), rp.ctypes.data_as(abi._ip), cj.ctypes.data_as(abi._ip),
                          int(seed) & (2 ** 64 - 1), cf.ctypes.data_as(abi._ip)))
    return cf


def interp(n, rowptr, col, val, s_rowptr, s_col, cf, interp_type=AMG_CLASSICAL_EXT_I, num_functions=1, device=-1):
    """amg_classical_interp: P of one level, (nrows, ncols, rowptr, col, val)."""
    from . import check, lib
    rp, cj, v = _csr_args(rowptr, col, val)
    srp, scj, _ = _csr_args(s_rowptr, s_col)
    c = np.ascontiguousarray(cf, dtype=np.int32)
    if rp.size != int(n) + 1 or srp.size != int(n) + 1 or c.size != int(n):
        raise ValueError("interp: rowptr / cf length")
    h = abi.AmgHostCsr()
    check(lib.amg_classical_interp(int(device), int(n), rp.ctypes.data_as(abi._ip), cj.ctypes.data_as(abi._ip),
                                   v.ctypes.data_as(abi._dp), srp.ctypes.data_as(abi._ip),
                                   scj.ctypes.data_as(abi._ip), c.ctypes.data_as(abi._ip), int(interp_type),
                                   int(num_functions), C.byref(h)))
    return _host_csr(h)


def set_setup_scratch(slots):
    """amg_set_setup_scratch: the device interpolation's scratch budget in
    slots per batch of rows, process-wide; 0 restores the default."""
    from . import check, lib
    check(lib.amg_set_setup_scratch(int(slots)))


class ClassicalAMG:
    """Hierarchy (held on the host) from a square CSR (diagonal first); keywords
    are the fields of amg_classical_opts, setup_on_device among them."""

    def __init__(self, n, rowptr, col, val, opts=None, **kw):
        from . import check, lib
        self._lib = lib
        o = opts if opts is not None else default_opts(**kw)
        rp = np.ascontiguousarray(rowptr, dtype=np.int32)
        cj = np.ascontiguousarray(col, dtype=np.int32)
        v = np.ascontiguousarray(val, dtype=np.float64)
        h = C.c_void_p()
        check(lib.amg_classical_setup(C.byref(o), int(n), rp.ctypes.data_as(abi._ip),
                                      cj.ctypes.data_as(abi._ip), v.ctypes.data_as(abi._dp), C.byref(h)))
        self.h = h
        self.L = lib.amg_classical_levels(h)

    def get(self, which, level):
        """(nrows, ncols, rowptr, col, val) numpy copies of operator which
        (AMG_GEN_A/P/R; AMG_GEN_PS/RS after smooth_transfers)."""
        from . import check
        nr, nc, nz = C.c_int(), C.c_int(), C.c_longlong()
        rp, cj, v = abi._ip(), abi._ip(), abi._dp()
        check(self._lib.amg_classical_get(self.h, which, level, C.byref(nr), C.byref(nc), C.byref(nz),
                                          C.byref(rp), C.byref(cj), C.byref(v)))
        n, z = nr.value, nz.value
        return (n, nc.value, np.ctypeslib.as_array(rp, (n + 1,)).copy(),
                np.ctypeslib.as_array(cj, (max(z, 1),))[:z].copy() if z else np.zeros(0, np.int32),
                np.ctypeslib.as_array(v, (max(z, 1),))[:z].copy() if z else np.zeros(0))

    def smooth_transfers(self, w, add_P_max_elmts=0, add_trunc_factor=0.0, device=-1):
        """amg_classical_smooth_transfers: build (or rebuild) every level's
        P~ = (I - w D^-1 A) P and R~, truncated when an add_* option is set
        (R~ is then the transpose of the truncated P~); get / register them as
        AMG_GEN_PS / AMG_GEN_RS."""
        from . import check
        check(self._lib.amg_classical_smooth_transfers(self.h, float(w), int(add_P_max_elmts),
                                                       float(add_trunc_factor), int(device)))

    def cf_marker(self, level):
        from . import check
        n = self.get(AMG_GEN_A, level)[0]
        cf = np.zeros(n, dtype=np.int32)
        check(self._lib.amg_classical_cf_marker(self.h, level, cf.ctypes.data_as(abi._ip)))
        return cf

    def register(self, ctx, which, level):
        from . import Mat, check
        h = C.c_void_p()
        check(self._lib.amg_classical_register(ctx.h, self.h, which, level, C.byref(h)))
        return Mat(ctx, h)

    def hierarchy(self, ctx, opts, levels=None, smoothed=False):
        """Register every level on the device and build a Hier (amg_hier_create);
        smoothed: the transfers are P~ / R~ of smooth_transfers (MULTADD)."""
        from . import Hier
        L = self.L if levels is None else levels
        As = [self.register(ctx, AMG_GEN_A, l) for l in range(L)]
        Ps = [self.register(ctx, AMG_GEN_PS if smoothed else AMG_GEN_P, l) for l in range(L - 1)]
        Rs = [self.register(ctx, AMG_GEN_RS if smoothed else AMG_GEN_R, l) for l in range(L - 1)]
        return Hier(ctx, As, Ps, Rs, opts)

    def free(self):
        if self.h:
            self._lib.amg_classical_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass
