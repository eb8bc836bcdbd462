"""The transform drivers of the C ABI (include/pdwt_hip.h) on buffers of a CALLER: every buffer guarded on both sides
(tests/cabi_arena.py), misaligned down to its element size or tightly packed, d_tmp full of arbitrary words.  Called through ctypes on
pdwt_amd.hip() directly, never through the Wavelets classes (whose buffers are all 256-byte aligned).

Per case of tests/cabi_cases.py (TRANSFORM_CASES), precision and layout (LAYOUTS): forward, inverse from the forward's own output, and
inverse from the reference coefficients.  After each call: return code 0; no byte outside a payload and no byte of a read-only payload
changed (the image for a forward; every band but band 0 for a 1-D / 2-D inverse, every band for a 3-D one); values within TOL of a
FLOAT64 reference (oracle.OracleWavelets / tests/ref3d.py; Haar bit for bit against the oracle in the same precision).  Band 0 is
allocated at its documented level-1 size and only its first pdwt_band_size(info, 0) elements are compared.

The (gate -> case) table is cabi_cases.GATES: for each row the launch counts (pdwt_ktime_read) of the aligned layout must show the
gated kernel, and those of every misaligned layout of the row must show it gone and its fallback launched, with all of the above
still holding.  Covered here: the separable, SWT, Haar and 3-D transform drivers; the utilities, statistics, non-separable and
batch2d entries are not."""
import ctypes as C

import numpy as np
import pytest

import pdwt_amd
from pdwt_amd import _native as nat
from tests import cabi_cases as M
from tests.cabi_arena import Arena, ArenaDamage, Region
from tests.helpers import TOL, band_err, knobs

pytestmark = pytest.mark.gpu

CT = {"f32": C.c_float, "f64": C.c_double}
DT = {"f32": np.dtype(np.float32), "f64": np.dtype(np.float64)}
DRV = {"dwt2": ("forward_separable", "inverse_separable"), "dwt1": ("forward_separable_1d", "inverse_separable_1d"),
       "swt2": ("forward_swt_separable", "inverse_swt_separable"), "swt1": ("forward_swt_separable_1d", "inverse_swt_separable_1d"),
       "haar2": ("haar_forward2d", "haar_inverse2d"), "haar1": ("haar_forward1d", "haar_inverse1d"),
       "dwt3": ("forward3d_separable", "inverse3d_separable"), "swt3": ("forward3d_swt", "inverse3d_swt")}
_PARAMS = [(c, s) for c in M.TRANSFORM_CASES for s in c["dtypes"]]


def _geometry(L, case, sfx, levels, hlen):
    """info, band sizes, the allocation of band 0, d_tmp elements, the two drivers' argument tails, the odd-one-out band numbers"""
    fam, shape = case["fam"], case["shape"]
    g = dict(fam=fam)
    if fam in ("dwt3", "swt3"):
        info = nat.Info3D(shape[0], shape[1], shape[2], levels, hlen)
        s = "3d" if fam == "dwt3" else "_swt3d"
        nb = getattr(L, "pdwt_num_bands" + s)(info)
        sizes = [int(getattr(L, "pdwt_band_size" + s)(info, k, None, None, None)) for k in range(nb)]
        g.update(alloc0=sizes[0], tmp=int(getattr(L, "pdwt_tmp_elems" + s)(info)), fine=nb - 1, coarse=1, keeps_band0=True)
        swt_filters = 0
    else:
        ndim = 1 if fam in ("dwt1", "swt1", "haar1") else 2
        swt = int(fam in ("swt2", "swt1"))
        info = nat.Info(ndim, shape[0], shape[1], levels, swt, hlen)
        nb = L.pdwt_num_bands(info)
        sizes = [int(L.pdwt_band_size(info, k, None, None)) for k in range(nb)]
        # [A_L, H1, V1, D1, ..., H_L, V_L, D_L] / [A_L, D1 .. D_L]: band 0 is allocated at the size of a level-1 band
        g.update(alloc0=sizes[1], tmp=int(L.pdwt_tmp_elems(info)), fine=2 if ndim == 2 else 1, coarse=nb - 2 if ndim == 2 else nb - 1, keeps_band0=False)
        swt_filters = swt
    assert nb > 1 and min(sizes) > 0 and g["tmp"] > 0, (case["id"], nb, sizes, g["tmp"])
    tail = [info]
    if not fam.startswith("haar"):
        f = {"f32": nat.Filters32, "f64": nat.Filters64}[sfx]()
        assert getattr(L, "pdwt_compute_filters_separable_" + sfx)(case["wname"].encode(), swt_filters, C.byref(f)) == hlen, case["id"]
        tail.append(C.byref(f))
        g["_keep"] = f
    g.update(info=info, nb=nb, sizes=sizes, tail=tail)
    return g


def _regions(g, sfx, layout):
    dt, mis = DT[sfx], lambda name: M.misalign(layout, name, g["fine"], g["coarse"])
    img = Region("image", g["n_image"], dt, "in", mis("image"))
    tmp = Region("tmp", g["tmp"], dt, "scratch", mis("tmp"))
    bands = [Region("band%d" % k, g["alloc0"] if k == 0 else g["sizes"][k], dt, "out", mis("band%d" % k)) for k in range(g["nb"])]
    return [img, tmp, bands] if layout == "packed" else [img, tmp] + bands


def _launches(L):
    n, ms, d = C.c_int(), C.c_double(), {}
    for k in range(L.pdwt_kernel_count()):
        L.pdwt_ktime_read(k, C.byref(n), C.byref(ms))
        if n.value:
            d[L.pdwt_kernel_name(k).decode()] = n.value
    return d


def _check_gates(case, sfx, prof, bad):
    """prof[(layout, 'fwd' | 'inv')] = {kernel name: launches}; the rows of GATES for this case"""
    for g in M.GATES:
        if g["case"] != case["id"] or g["dt"] != sfx:
            continue
        al = prof[("aligned", g["dir"])]
        if not all(al.get(k, 0) >= 1 for k in g["fast"]):
            bad.append("gate %s: aligned layout did not launch %s: %s" % (g["gate"], g["fast"], al))
        if not g["fast_gone"] and any(al.get(k, 0) for k in g["slow"]):
            bad.append("gate %s: aligned layout launched the fallback %s: %s" % (g["gate"], g["slow"], al))
        for layout in g["flips"]:
            if (layout, g["dir"]) not in prof:
                continue  # all+2 is a float32 layout
            p = prof[(layout, g["dir"])]
            if any(p.get(k, 0) for k in g["fast_gone"]) or not any(p.get(k, 0) for k in g["slow"]):
                bad.append("gate %s: layout %s did not flip %s -> %s: %s" % (g["gate"], layout, g["fast_gone"], g["slow"], p))


@pytest.mark.parametrize("case,sfx", _PARAMS, ids=["%s-%s" % (c["id"], s) for c, s in _PARAMS])
def test_transform_drivers_on_guarded_misaligned_buffers(case, sfx):
    L = pdwt_amd.hip()
    dt, ct, fam = DT[sfx], CT[sfx], case["fam"]
    haar = fam.startswith("haar")
    levels, hlen, rbands, rrec = M.reference(case, dt if haar else M.F64)
    x = M.case_input(case).astype(dt)
    g = _geometry(L, case, sfx, levels, hlen)
    g["n_image"] = x.size
    assert len(rbands) == g["nb"] and [b.size for b in rbands] == g["sizes"], (case["id"], [b.size for b in rbands], g["sizes"])
    fwd, inv = [getattr(L, "pdwt_%s_%s" % (d, sfx)) for d in DRV[fam]]
    names = ["band%d" % k for k in range(g["nb"])]
    junk = np.full(x.size, 7.0, dtype=dt)
    bad, prof = [], {}

    def same(got, ref, what):
        if haar:
            if not np.array_equal(got, np.asarray(ref, dtype=dt).reshape(-1)):
                bad.append("%s: not bit-identical to the oracle (err %.3g)" % (what, band_err(got, np.asarray(ref).reshape(-1))))
        else:
            e = band_err(got, np.asarray(ref).reshape(-1))
            if not e <= TOL[dt]:
                bad.append("%s: error %.3g > %.1g" % (what, e, TOL[dt]))

    def run(A, fn, ctx):
        L.pdwt_ktime_reset()
        rc = fn(A.ptr("image"), A.band_table(names, ct), A.ptr("tmp"), *g["tail"])
        assert L.pdwt_sync() == 0 and rc == 0, (ctx, rc, L.pdwt_last_error_string())  # a failed launch ends the test at once
        counts = _launches(L)
        try:
            return A.check(ctx), counts
        except ArenaDamage as e:
            bad.append(str(e))
            return A.host, counts

    with knobs(**case["knobs"]):
        L.pdwt_ktime_enable(1)
        try:
            for layout in M.LAYOUTS:
                if layout == "all+2" and sfx != "f32":
                    continue
                ctx = "%s %s %s" % (case["id"], sfx, layout)
                A = Arena(L, _regions(g, sfx, layout), {"image": x})
                try:
                    image, prof[(layout, "fwd")] = run(A, fwd, ctx + " forward")
                    for k in range(g["nb"]):
                        same(A.get(image, names[k], g["sizes"][k]), rbands[k], ctx + " forward band %d" % k)
                    # inverse: the image is written, band 0 may be clobbered (1-D / 2-D), every other band must survive
                    A.by_name["image"].role = "out"
                    for k in range(g["nb"]):
                        A.by_name[names[k]].role = "in" if (k or g["keeps_band0"]) else "inout"
                    A.upload("image", junk)
                    image, prof[(layout, "inv")] = run(A, inv, ctx + " inverse of own output")
                    same(A.get(image, "image"), rrec, ctx + " inverse of own output")
                    A.upload("image", junk)
                    for k in range(g["nb"]):
                        A.upload(names[k], np.asarray(rbands[k], dtype=dt))
                    image, _ = run(A, inv, ctx + " inverse of reference coefficients")
                    same(A.get(image, "image"), rrec, ctx + " inverse of reference coefficients")
                finally:
                    A.free()
        finally:
            L.pdwt_ktime_enable(0)
            L.pdwt_ktime_reset()
    for key in sorted(prof):
        print("%s %-8s %s: %s" % (case["id"], key[0], key[1], prof[key]))
    _check_gates(case, sfx, prof, bad)
    assert not bad, "\n".join(bad)
