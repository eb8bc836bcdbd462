"""The case matrix of the guard-zone / misaligned-buffer tests of the C ABI (include/pdwt_hip.h) as plain data, importable without a
GPU: layouts, transform cases, the (gate -> case) table, and the inputs and float64 references the cases share.
tests/test_cabi_buffers_gpu.py walks the matrix on tests/cabi_arena.py arenas and asserts the launch profiles of GATES;
tests/test_cabi_cases_cpu.py checks on the CPU that the matrix is consistent and that the float32 bar (TOL against a float64
reference) is reachable for every transform case."""
import numpy as np

F32, F64 = np.dtype(np.float32), np.dtype(np.float64)

# ---- layouts ---------------------------------------------------------------------------------------------------------------------
# name -> which regions start one (two) element(s) past a 256-byte boundary.  fine / coarse: ONE detail band of the finest / coarsest
# level is the odd one out (the cascade gates treat A2 and the detail bands separately).  packed: the bands back to back in band
# order, guards at the two ends only.  all+2 (8-byte but not 16-byte aligned) is a float32 layout.
LAYOUTS = ["aligned", "image+1", "tmp+1", "bands+1", "band0+1", "fine+1", "coarse+1", "all+1", "all+2", "packed"]


def misalign(layout, name, fine, coarse):
    """elements of misalignment of region `name` under `layout`; fine / coarse: band numbers of the two odd-one-out layouts"""
    if layout in ("aligned", "packed"):
        return 0
    if layout == "all+1":
        return 1
    if layout == "all+2":
        return 2
    band = name.rsplit("band", 1)[-1] if "band" in name else None
    return int({"image+1": name.endswith("image"), "tmp+1": name.endswith("tmp"), "bands+1": band is not None, "band0+1": band == "0",
                "fine+1": band == str(fine), "coarse+1": band == str(coarse)}[layout])


# ---- transform cases -----------------------------------------------------------------------------------------------------------
# fam: dwt2 / dwt1 / swt2 / swt1 (the separable drivers), haar2 / haar1, dwt3 / swt3.  dtypes: "f32", "f64" or both.  knobs: pdwt_debug_set values held while the case runs.
def _c(cid, fam, shape, wname, levels, dtypes=("f32", "f64"), **kn):
    return dict(id=cid, fam=fam, shape=shape, wname=wname, levels=levels, dtypes=dtypes, knobs=kn)


TRANSFORM_CASES = [
    # float32 streaming level kernels (dwt_stream.hip): even nr, nc % 4 == 0, nc >= 64, nr >= 2 * hlen, even hlen 4..16
    _c("stream64-db2-L1", "dwt2", (64, 64), "db2", 1, ("f32",), casc=0),
    _c("stream64-db4-L2", "dwt2", (64, 64), "db4", 2, ("f32",), casc=0),
    _c("stream72x96-db8-L1", "dwt2", (72, 96), "db8", 1, ("f32",), casc=0),
    _c("stream72x96-db2-L2", "dwt2", (72, 96), "db2", 2, ("f32",), casc=0),
    # float32 cascade pairs / three-level inverse (dwt_casc*.hip): casc_min = 0, the smallest size whose t1 is the trash area
    # (Scratch::t1_is_trash: Nr * ceil(Nc / 2) >= 256 * 1024)
    _c("casc512x1024-db4-L2", "dwt2", (512, 1024), "db4", 2, ("f32",), casc_min=0),             # inverse: dwt_casc_inv3.hip, two-level form
    _c("casc512x1024-db4-L2-invw", "dwt2", (512, 1024), "db4", 2, ("f32",), casc_min=0, casc_l3=2),  # inverse: dwt_casc_invw.hip
    _c("casc512x1024-db4-L2-iwg1", "dwt2", (512, 1024), "db4", 2, ("f32",), casc_min=0, casc_iwg=1),  # inverse: inv2d_casc_f32 (dwt_casc.hip)
    _c("casc512x1024-db2-L3", "dwt2", (512, 1024), "db2", 3, ("f32",), casc_min=0),             # inverse: three levels streamed (inv3)
    _c("casc512x1024-db2-L3-invw", "dwt2", (512, 1024), "db2", 3, ("f32",), casc_min=0, casc_l3=2),  # inverse: three levels, invw with l3
    _c("casc512x1024-db2-L3-nol3", "dwt2", (512, 1024), "db2", 3, ("f32",), casc_min=0, casc_l3=0),  # inverse: one level + a pair
    _c("casc512x1024-db2-L4", "dwt2", (512, 1024), "db2", 4, ("f32",), casc_min=0),             # pairs whose output is a ping buffer of d_tmp
    # dwt_lds.hip: double precision with any even bank, float32 with more than 16 taps; odd sizes; a zero-padded length (db5)
    _c("lds96x128-db4-L2", "dwt2", (96, 128), "db4", 2, ("f64",), f64_lds_min=0),
    _c("lds97x131-db5-L2", "dwt2", (97, 131), "db5", 2, ("f64",), f64_lds_min=0),
    _c("lds96x128-db10-L1", "dwt2", (96, 128), "db10", 1, ("f32", "f64"), f64_lds_min=0),
    _c("lds97x131-sym13-L1", "dwt2", (97, 131), "sym13", 1, ("f32",), f64_lds_min=0),
    # dwt_lat.hip: the lattice level kernels of the orthogonal double-precision banks
    _c("lat256-db4-L1", "dwt2", (256, 256), "db4", 1, ("f64",), f64_lat_min=256),
    _c("lat256-db20-L1", "dwt2", (256, 256), "db20", 1, ("f64",), f64_lat_min=256),
    # tiled fused level kernels (odd sizes keep float32 off the streaming kernels) and the two-pass kernels
    _c("tiled50x37-db3-L2", "dwt2", (50, 37), "db3", 2),
    _c("tiled64-db4-L2", "dwt2", (64, 64), "db4", 2, stream=0, casc=0, f64_lds=0),
    _c("twopass50x37-sym4-L2-tr0", "dwt2", (50, 37), "sym4", 2, force_twopass=1, rows_tr=0),
    _c("twopass64-db10-L1-tr1", "dwt2", (64, 64), "db10", 1, force_twopass=1, rows_tr=1),
    _c("twopass64-db4-L2-tr1", "dwt2", (64, 64), "db4", 2, force_twopass=1, rows_tr=1),
    # batched 1-D (dwt1d_fused.hip; the float64 one-buffer kernels at long rows; the per-level row kernels)
    _c("b1d-5x256-sym8-L4", "dwt1", (5, 256), "sym8", 4),
    _c("b1d-3x77-db3-L2", "dwt1", (3, 77), "db3", 2),
    _c("b1d-8x8192-db4-L3", "dwt1", (8, 8192), "db4", 3, ("f64",)),
    _c("b1d-8x8192-db4-L3-rows", "dwt1", (8, 8192), "db4", 3, ("f64",), dwt1d_f64=0),
    _c("b1d-5x256-db2-L3-twopass", "dwt1", (5, 256), "db2", 3, force_twopass=1),
    # SWT: tap spacings 1, 2, 4; fused / two-pass; residue-major rows; long banks; double precision
    _c("swt64-db2-L3", "swt2", (64, 64), "db2", 3),
    _c("swt64-db2-L3-noperm", "swt2", (64, 64), "db2", 3, ("f32",), swtf_perm=0),
    _c("swt64-db2-L3-twopass", "swt2", (64, 64), "db2", 3, swtf=0),
    _c("swt50x70-db3-L2", "swt2", (50, 70), "db3", 2),
    _c("swt96x128-sym13-L1", "swt2", (96, 128), "sym13", 1, ("f32",)),
    _c("swt96x128-db20-L1", "swt2", (96, 128), "db20", 1, ("f32",)),
    _c("swt64-db3-L2-f64-twopass", "swt2", (64, 64), "db3", 2, ("f64",), swtf_f64=0),
    _c("swt1d-6x128-sym4-L3", "swt1", (6, 128), "sym4", 3),
    # Haar: the vector form (float32, nc % 4 == 0, even nr), odd sizes, 1-D
    _c("haar64-L2", "haar2", (64, 64), "haar", 2),
    _c("haar37x51-L2", "haar2", (37, 51), "haar", 2),
    _c("haar1d-3x77-L3", "haar1", (3, 77), "haar", 3),
    _c("haar1d-4x64-L2", "haar1", (4, 64), "haar", 2),
    # volumes
    _c("dwt3-20x24x28-db2-L2", "dwt3", (20, 24, 28), "db2", 2),
    _c("dwt3-19x22x27-sym4-L1", "dwt3", (19, 22, 27), "sym4", 1),
    _c("swt3-20x24x28-db2-L2", "swt3", (20, 24, 28), "db2", 2),
    _c("swt3-19x22x27-sym4-L1", "swt3", (19, 22, 27), "sym4", 1),
]
CASE_BY_ID = {c["id"]: c for c in TRANSFORM_CASES}
FAMILIES = ["dwt2", "dwt1", "swt2", "swt1", "haar2", "haar1", "dwt3", "swt3"]

# ---- (gate -> case) ---------------------------------------------------------------------------------------------------------------
# One row per host-side pointer gate of `grep -n "& 15" pdwt_amd/csrc` (al16 / aligned16 / b2_al16 are the same test).  The aligned
# layout of `case` must show every kernel of `fast` launched (count >= 1) and none of `slow`; every layout of `flips`, at the same
# shape and knobs, must show every kernel of `fast_gone` not launched and one of `slow` (the fallbacks) launched, and still satisfy
# assertions 1-5.  Kernel names: pdwt_kernel_name; "stat_*": the pdwt_debug_get counters.  Where the gated kernel shares its timer id
# with its fallback (the fused SWT levels are timed as swt_*_cols) the row kernels, which only the two-pass fallback launches, are the
# evidence: `slow` with an empty `fast_gone`.  (fwd2d_f64 / inv2d_f64 are the LDS level kernels of dwt_lds.hip, which take a 512x1024
# float32 level once the cascade and the streaming kernel have both refused it.)
def _g(gate, case, dt, direction, flips, fast=(), slow=(), fast_gone=None):
    return dict(gate=gate, case=case, dt=dt, dir=direction, flips=flips, fast=tuple(fast), slow=tuple(slow),
                fast_gone=tuple(fast if fast_gone is None else fast_gone))


_ANY = ("image+1", "bands+1", "band0+1", "fine+1", "all+1", "all+2")
_CASC = ("image+1", "bands+1", "fine+1", "all+1", "all+2")
_SWT = ("image+1", "tmp+1", "bands+1", "fine+1", "all+1", "all+2")
GATES = [
    _g("dwt_stream.hip:500 fwd2d_stream_f32", "stream64-db2-L1", "f32", "fwd", _ANY, fast=["fwd2d_stream"], slow=["fwd2d_fused"]),
    _g("dwt_stream.hip:515 inv2d_stream_f32", "stream64-db2-L1", "f32", "inv", _ANY, fast=["inv2d_stream"], slow=["inv2d_fused"]),
    _g("dwt_casc.hip:1008 fwd2d_casc_f32", "casc512x1024-db4-L2", "f32", "fwd", _CASC + ("band0+1", "coarse+1"), fast=["fwd2d_casc"],
       slow=["fwd2d_stream", "fwd2d_fused", "fwd2d_f64"]),
    _g("dwt_casc_inv3.hip:837 inv2d_casc3_f32 (three levels)", "casc512x1024-db2-L3", "f32", "inv", _CASC + ("tmp+1",), fast=["inv2d_casc"],
       slow=["inv2d_stream", "inv2d_fused", "inv2d_f64"]),
    _g("dwt_casc_inv3.hip:838 inv2d_casc3_f32 (pair: A2)", "casc512x1024-db4-L2", "f32", "inv", _CASC + ("tmp+1", "band0+1", "coarse+1"), fast=["inv2d_casc"],
       slow=["inv2d_stream", "inv2d_fused", "inv2d_f64"]),
    _g("dwt_casc_invw.hip:516 inv2d_cascw_f32 (three levels)", "casc512x1024-db2-L3-invw", "f32", "inv", _CASC + ("tmp+1",), fast=["inv2d_casc"],
       slow=["inv2d_stream", "inv2d_fused", "inv2d_f64"]),
    _g("dwt_casc_invw.hip:517 inv2d_cascw_f32 (pair: A2)", "casc512x1024-db4-L2-invw", "f32", "inv", _CASC + ("tmp+1", "band0+1", "coarse+1"), fast=["inv2d_casc"],
       slow=["inv2d_stream", "inv2d_fused", "inv2d_f64"]),
    _g("dwt_casc.hip:1066 inv2d_casc_f32", "casc512x1024-db4-L2-iwg1", "f32", "inv", _CASC + ("tmp+1", "band0+1", "coarse+1"), fast=["inv2d_casc"],
       slow=["inv2d_stream", "inv2d_fused", "inv2d_f64"]),
    _g("swt_fused.inc:617 swt_fwd_fused_f32", "swt64-db2-L3", "f32", "fwd", _SWT, fast=["swt_ana_cols"], fast_gone=[], slow=["swt_ana_rows"]),
    _g("swt_fused.inc:685 swt_inv_fused_f32", "swt64-db2-L3", "f32", "inv", _SWT, fast=["swt_syn_cols"], fast_gone=[], slow=["swt_syn_rows"]),
    _g("swt_fused_f64.inc:306 swt_fwd_fused_f64", "swt64-db2-L3", "f64", "fwd", _SWT, fast=["swt_ana_cols"], fast_gone=[], slow=["swt_ana_rows"]),
    _g("swt_fused_f64.inc:341 swt_inv_fused_f64", "swt64-db2-L3", "f64", "inv", _SWT, fast=["swt_syn_cols"], fast_gone=[], slow=["swt_syn_rows"]),
]

# Not in GATES: the gates that choose between two kernels of ONE timer id (swt.hip:248 swt_rows_lds, haar.hip:182,201, rows_tr.hip:108,223,
# cols_ring.inc:571, dwt1d_fused.hip:801-862) and the in-kernel `vec` / `vec_ok` branches of dwt1d_fused.hip -- no launch count can
# tell their sides apart.  Their cases run under every layout and must be correct; each has element counts divisible by the vector
# width (then the pointer is the only reason the scalar side runs) and a neighbour that is not.  (branch -> cases)
VEC_BRANCHES = {
    "dwt1d_fused.hip:155,205,339,532,552 (rowvec / vec_ok)": ["b1d-5x256-sym8-L4", "b1d-3x77-db3-L2"],
    "dwt1d_fused.hip:801,815,840,844,859,862 (float64 one-buffer / prefetch forms)": ["b1d-8x8192-db4-L3", "b1d-8x8192-db4-L3-rows"],
    "rows_tr.hip:108,223": ["twopass64-db10-L1-tr1", "twopass64-db4-L2-tr1", "twopass50x37-sym4-L2-tr0"],
    "swt.hip:248 swt_rows_lds": ["swt64-db2-L3-twopass", "swt64-db3-L2-f64-twopass", "swt50x70-db3-L2", "swt1d-6x128-sym4-L3"],
    "haar.hip:182,201 (vector form)": ["haar64-L2", "haar37x51-L2"],
    "cols_ring.inc:571": ["twopass64-db4-L2-tr1", "swt64-db2-L3-twopass"],
}


def case_input(case):
    """the input of a transform case: float32 values (exact in float64 too, so both precisions and the reference see the same image)"""
    rs = np.random.RandomState(sum(map(ord, case["id"])))
    return rs.uniform(-1, 1, case["shape"]).astype(np.float32)


def oracle_for(case, dtype):
    """the oracle object of a 1-D / 2-D case on the case's input in `dtype`, forward done"""
    from oracle import oracle as orc
    fam = case["fam"]
    x = case_input(case).astype(dtype)
    swt = int(fam in ("swt2", "swt1"))
    ndim = 1 if fam in ("dwt1", "swt1", "haar1") else 2
    O = orc.OracleWavelets(x, case["wname"], case["levels"], do_swt=swt, ndim=ndim)
    O.forward()
    return O


_REF = {}


def reference(case, dtype=F64):
    """(levels, hlen, [bands], reconstruction) of a case, computed once.  float64 for everything but Haar, which is pinned bit for bit to
    the oracle in the dtype under test."""
    key = (case["id"], np.dtype(dtype).name)
    if key not in _REF:
        fam = case["fam"]
        if fam in ("dwt3", "swt3"):
            from tests import ref3d
            x = case_input(case).astype(np.float64)
            L = ref3d.levels_of(case["shape"], case["wname"], case["levels"])
            hlen = len(ref3d.bank(case["wname"], 0)[0])
            if fam == "dwt3":
                c = ref3d.dwt3_forward(x, case["wname"], L)
                r = ref3d.dwt3_inverse(c, x.shape, case["wname"], L)
            else:
                c = ref3d.swt3_forward(x, case["wname"], L)
                r = ref3d.swt3_inverse(c, case["wname"], L)
            _REF[key] = (L, hlen, [np.asarray(b) for b in c], np.asarray(r))
        else:
            O = oracle_for(case, dtype)
            c = O.coeffs
            O.inverse()
            _REF[key] = (O.info.nlevels, O.info.hlen, c, O.get_image())
    return _REF[key]
