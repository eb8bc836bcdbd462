"""The (kernel family x filter bank) matrix of the 1-D / 2-D transforms of ``pdwt_amd.Wavelets`` as plain data, importable without
a GPU.  tests/test_all_banks_gpu.py walks it on the device; tests/test_bank_matrix_cpu.py ties it to the sources (the X-macro lists
of pdwt_amd/csrc are parsed there and compared with FAMILY_LENGTHS) and checks that the float32 bar is reachable for every case.

One ROW per kernel family (and knob set that forces it).  A row says
  kind / dtypes / knobs   what runs: "dwt2" | "swt2" | "dwt1" | "swt1"; the pdwt_debug_set values held while a case runs
  accepts(hlen)           the bank lengths the family takes under these knobs
  inst                    {direction: [E(template, list, mapping, proof)]}: the kernel templates a bank of the row may run on, the
                          FAMILY_LENGTHS list each is instantiated from, the mapping of a bank length onto it -- "exact" (the bank's
                          own length), "pad8" / "pad_l2" (the next multiple of 8 / of 24-32-40, zero-padded) or "generic" (lengths
                          outside the list run the run-time-length template, H = 0) -- and the evidence that proves it ran.  Coverage
                          is counted per (template, precision, instantiated length): TEMPLATES, case_reaches
  shapes(hlen, L)         the smallest shapes that pass the family's gates at every one of the L levels (derived from the gates
                          quoted beside each rule; where a family takes odd sizes: one even and one odd shape)
  levels / levels2        the level count of the sweep over all banks / the second one, run for one bank per length
  evidence(hlen, L, shape, direction) -> (ran, quiet): kernel timer names (pdwt_kernel_name) and "stat_*" launch counters
                          (pdwt_debug_get) that must show at least one launch / none at all
  pad_check, pad_evidence (knob, value) under which other kernels run the banks of a padded instantiation, and the launch evidence of
                          that: bands bit-identical

What the launchers' gates say, as derived for the shape rules:
  * the tiled fused kernels (dwt.hip) are never launched in double precision: fwd_fused_lds / inv_fused_lds pass the 64 KiB budget
    from 4 taps on (70 KB / 73 KB); double precision with f64_lds = 0 runs the two-pass kernels.  In float32 the forward fits up to 26
    taps and the inverse up to 34, so the 30-tap instantiation is reachable through the inverse only and the 40-tap one not at all;
    k_ana_rows / k_ana_cols / k_syn_* use the same list and reach every length of it.
  * dwt_lds.hip takes EVERY even float32 length once the streaming kernels are off (knob stream = 0), not only banks over 16 taps.
  * dwt_casc_inv3.hip and dwt_casc_invw.hip decline 512 x 1024 under the default knobs: their launchers want one workgroup per CU, at
    most half as many, and every wave at least hlen / 2 coefficient rows (inv3_fits / invw_fits below replay them; the smallest
    images they take by default have 0.8 .. 3.5 M pixels).  Their rows therefore set knob casc_iwaves = 256 -- a target of 16 resp. 32
    workgroups instead of one per CU -- under which the smallest image the forward cascade takes, 512 x 1024 (taller
    where nr >= 32 hlen asks for it), is taken in the two-level form; inv2d_casc_f32 (casc_iwg = 1) takes it as it is.
  * the three-level form of dwt_casc_invw.hip fits no bank of more than 12 taps (kInvA2Rows / kInvR3Max); its L = 3 cases run one level
    kernel and the two-level form there.
  * the lattice kernels (dwt_lat.hip, 40 taps) take db20 only: sym20 has no lattice table.
  * the one-buffer kernels of the batched 1-D transform (dwt1d_fused.hip, double precision, rows over the LDS budget): the forward is
    instantiated up to 20 taps, the inverse for every length, and needs three levels or more at 8192 samples.
Not counted per template: the tap-spacing variants of the fused SWT kernels (<HLEN, F>; the rows run three levels, spacings 1, 2, 4),
the workgroup shapes of the cascade kernels (<HLEN, NV, W>) and the prefetch / vector variants of the 1-D kernels.
"""
import numpy as np

from tests.helpers import load_golden
from tests import ref3d

F32, F64 = np.dtype(np.float32), np.dtype(np.float64)
ALL72 = [str(n) for n in load_golden("all72_1d_2x256_L1")["names"]]


def ev(a, b):
    return list(range(a, b + 1, 2))


# ---- the instantiated tap counts, as the sources list them (checked by tests/test_bank_matrix_cpu.py) -------------------------------
FAMILY_LENGTHS = {
    "PDWT_STREAM_FWD_HLENS": ev(4, 16), "PDWT_STREAM_INV_HLENS": ev(4, 16),
    "PDWT_CASC_FWD_HLENS": ev(4, 20), "PDWT_CASC_INV_HLENS": ev(4, 10), "PDWT_CASCW_INV_HLENS": ev(4, 18),
    "inv2d_casc3_f32": [4, 8, 12, 16, 20],
    "PDWT_TILED_HLENS": ev(4, 20) + [24, 30, 40], "PDWT_F64LDS_HLENS": [8, 16, 24, 32, 40], "PDWT_LAT_HLENS": [40],
    "PDWT_1D_HLENS": ev(4, 40), "PDWT_ROWS_TR_HLENS": [20, 24, 30, 40], "PDWT_RING_HLENS": ev(12, 20) + [24, 30, 40],
    "PDWT_SWT_RING_HLENS": ev(2, 20), "PDWT_SWT_ROWS_HLENS": ev(2, 20),
    "PDWT_SWTF_HLENS:1": ev(2, 16), "PDWT_SWTF_HLENS:3": ev(8, 16), "PDWT_SWTF_HLENS:4": [18, 20],
    "PDWT_SWTL2_HLENS": [24, 32, 40], "PDWT_SWTD_HLENS": ev(2, 16),
}
# where each list lives: key -> (file, macro or function, preprocessor branch of the shipped build)
FAMILY_SOURCES = {
    "PDWT_STREAM_FWD_HLENS": ("dwt_stream.hip", "PDWT_STREAM_FWD_HLENS", None), "PDWT_STREAM_INV_HLENS": ("dwt_stream.hip", "PDWT_STREAM_INV_HLENS", None),
    "PDWT_CASC_FWD_HLENS": ("dwt_casc.hip", "PDWT_CASC_FWD_HLENS", "else"), "PDWT_CASC_INV_HLENS": ("dwt_casc.hip", "PDWT_CASC_INV_HLENS", "else"),
    "PDWT_CASCW_INV_HLENS": ("dwt_casc_invw.hip", "PDWT_CASCW_INV_HLENS", None), "inv2d_casc3_f32": ("dwt_casc_inv3.hip", "inv2d_casc3_f32", "switch"),
    "PDWT_TILED_HLENS": ("dwt.hip", "PDWT_TILED_HLENS", None), "PDWT_F64LDS_HLENS": ("dwt_lds.hip", "PDWT_F64LDS_HLENS", None),
    "PDWT_LAT_HLENS": ("dwt_lat.hip", "PDWT_LAT_HLENS", None), "PDWT_1D_HLENS": ("dwt1d_fused.hip", "PDWT_1D_HLENS", None),
    "PDWT_ROWS_TR_HLENS": ("rows_tr.hip", "PDWT_ROWS_TR_HLENS", None), "PDWT_RING_HLENS": ("cols_ring.inc", "PDWT_RING_HLENS", None),
    "PDWT_SWT_RING_HLENS": ("cols_ring.inc", "PDWT_SWT_RING_HLENS", None), "PDWT_SWT_ROWS_HLENS": ("swt.hip", "PDWT_SWT_ROWS_HLENS", None),
    # swt_fused.inc is compiled five times (PDWT_SWTF_PART 1 .. 5): parts 1 / 2 = forward / inverse of 2 .. 16 taps, 3 = the residue-major
    # inverse, 4 / 5 = forward / inverse of 18 and 20 taps
    "PDWT_SWTF_HLENS:1": ("swt_fused.inc", "PDWT_SWTF_HLENS", "if"), "PDWT_SWTF_HLENS:3": ("swt_fused.inc", "PDWT_SWTF_HLENS", "elif"),
    "PDWT_SWTF_HLENS:4": ("swt_fused.inc", "PDWT_SWTF_HLENS", "else"),
    "PDWT_SWTL2_HLENS": ("swt_fused_l2.inc", "PDWT_SWTL2_HLENS", None), "PDWT_SWTD_HLENS": ("swt_fused_f64.inc", "PDWT_SWTD_HLENS", None),
}


def hlen_of(wname):
    return len(ref3d.bank(wname)[0])


def one_bank_per_length():
    """the first bior / rbio bank of every filter length that has one, otherwise the first sym bank, otherwise the first bank (the
    rule of tests/test_3d_all_banks_gpu.py)"""
    by_len = {}
    for n in ALL72:
        by_len.setdefault(hlen_of(n), []).append(n)
    out = []
    for h in sorted(by_len):
        pick = [n for n in by_len[h] if n.startswith(("bior", "rbio"))] or [n for n in by_len[h] if n.startswith("sym")] or by_len[h]
        out.append(pick[0])
    return out


def pad8(h):
    return (h + 7) // 8 * 8


def pad_l2(h):
    return 24 if h <= 24 else (32 if h <= 32 else 40)


def instantiation(key, mapping, hlen):
    """the member of FAMILY_LENGTHS[key] a bank of hlen taps runs on (0: the generic template; None: the list does not serve it)"""
    lens = FAMILY_LENGTHS[key]
    if mapping == "exact":
        return hlen if hlen in lens else None
    if mapping == "generic":
        return hlen if hlen in lens else 0
    t = pad8(hlen) if mapping == "pad8" else pad_l2(hlen)
    return t if t in lens else None


# ---- gates replayed from the launchers ------------------------------------------------------------------------------------------
def _casc_inv_geom(h):  # CascInvGeom, casc_dev.hpp
    H2 = h // 2
    C = H2 // 2
    nbt = ((C + 1) // 2 if C > 0 else 0) + C
    return H2, 64 - 2 * nbt


def _g_range(strips, wgs=256):
    g = max(1, wgs // strips)
    return range(g, max(1, wgs // strips // 2) - 1, -1)


CASC_IWAVES = 256  # knob casc_iwaves of the two streamed inverse rows: a target of 16 workgroups (inv3: 256 / 16 waves) resp. 32 (invw: 256 / 8)


def inv3_fits(nr, nc, h, wgs=256):
    """launch_inv_casc3 (dwt_casc_inv3.hip): (W, gy) or None; gates of inv2d_casc3_f32 included.  wgs: the workgroup target, 256 (one per
    CU) unless knob casc_iwaves is set: ceil(casc_iwaves / 16)"""
    if (nr & 7) or (nc & 7) or nc < 256 or nr < 32 * h or h not in FAMILY_LENGTHS["inv2d_casc3_f32"]:
        return None
    H2, maxvl = _casc_inv_geom(h)
    np_, strips, reg = nr // 8, -(-(nc // 2) // (maxvl * 2)), (h // 2 - 1) * 64 * 48

    def fits(w, g):
        if (w - 1) * reg > 150 * 1024:
            return False
        for rp in (np_ // g, -(-np_ // g)):
            basep, remp = rp // w, rp % w
            if 2 * basep < H2 or rp - ((w - 1) * basep + min(w - 1, remp)) < 1:
                return False
        return True
    for w in (16, 16, 12, 8, 4):
        for g in _g_range(strips, wgs):
            if fits(w, g):
                return w, g
    return None


def invw_fits(nr, nc, h, l3, wgs=256):
    """launch_inv_cascw (dwt_casc_invw.hip): (W, gy) or None; gates of inv2d_cascw_f32 included; wgs: 256 or ceil(casc_iwaves / 8)"""
    m = 7 if l3 else 3
    if (nr & m) or (nc & m) or nc < 256 or nr < 32 * h or h not in FAMILY_LENGTHS["PDWT_CASCW_INV_HLENS"]:
        return None
    H2, maxvl = _casc_inv_geom(h)
    xs, nr2, strips, reg = H2 // 2, nr // 4, -(-(nc // 2) // (maxvl * 2)), (h // 2 - 1) * 64 * 48

    def fits(w, g):
        if (w - 1) * reg + (w * 16 * 256 if l3 else 0) > 150 * 1024:
            return False
        for R in (nr2 // g, -(-nr2 // g)):
            if R // w < H2:
                return False
            if l3:
                E = min(xs, R // w - 1)
                base, rem = (R + E) // w, (R + E) % w
                mid, lw = base + (1 if rem else 0), R - ((w - 1) * base + min(w - 1, rem))
                na2 = max(mid, lw + H2 - 1 + xs)
                if na2 > 16 or (na2 + 1) // 2 + 1 + H2 - 1 > 12:
                    return False
        return True
    for w in (8, 8, 16, 4):
        for g in _g_range(strips, wgs):
            if fits(w, g):
                return w, g
    return None


def casc_fwd_takes(nr, nc, h):
    """fwd2d_casc_f32 + Scratch::t1_is_trash (dwt.hip): the forward cascade launches whenever these hold"""
    return not (nr & 3) and not (nc & 3) and nc >= 256 and nr >= 16 * h and nr * ((nc + 1) // 2) >= 256 * 1024 and h in FAMILY_LENGTHS["PDWT_CASC_FWD_HLENS"]


def inv2_takes(nr, nc, h):
    """inv2d_casc_f32 (dwt_casc.hip)"""
    return not (nr & 3) and not (nc & 3) and nc >= 256 and nr >= 32 * h and nr * ((nc + 1) // 2) >= 256 * 1024 and h in FAMILY_LENGTHS["PDWT_CASC_INV_HLENS"]


_CASC_SHAPE = {}


def casc_shape(form, h):
    """the smallest image (by area, then rows) of 1024 .. 4096 columns that the forward cascade and inverse form `form` take, in the
    two-level form and -- where the family has one for this length -- the three-level form"""
    if (form, h) not in _CASC_SHAPE:
        def ok(nr, nc):
            if not casc_fwd_takes(nr, nc, h):
                return False
            if form == "inv3":
                return inv3_fits(nr, nc, h, CASC_IWAVES // 16) is not None  # (the same launcher serves both forms)
            if form == "invw":
                return invw_fits(nr, nc, h, False, CASC_IWAVES // 8) is not None and (h > 12 or not (nr & 7 or nc & 7) and invw_fits(nr, nc, h, True, CASC_IWAVES // 8) is not None)
            return inv2_takes(nr, nc, h)
        best = None
        for nc in (1024, 2048, 3072, 4096):
            for nr in range(512, 8193, 8):
                if best is not None and nr * nc >= best[0] * best[1]:
                    break
                if ok(nr, nc):
                    best = (nr, nc)
                    break
        assert best is not None, (form, h)
        _CASC_SHAPE[(form, h)] = best
    return _CASC_SHAPE[(form, h)]


def fused_lds_bytes(h, itemsize, inverse):
    """fwd_fused_lds / inv_fused_lds (dwt.hip; FTX = 64, FTY = 16): the tiled fused kernels run while this is <= 64 KiB"""
    if not inverse:
        rin, cinp = 2 * 16 + h - 2, (2 * 64 + h - 2) | 1
        return (rin * cinp + 2 * rin * 64) * itemsize
    h2 = h // 2
    rc, ccp = 16 + h2, (64 + h2) | 1
    return (4 * rc * ccp + 2 * 32 * ccp) * itemsize


def tiled_fused_takes(h, itemsize, inverse):
    return fused_lds_bytes(h, itemsize, inverse) <= 64 * 1024


# ---- shapes ----------------------------------------------------------------------------------------------------------------------
def _clamp_side(h, L):
    """the level clamp: N // (hlen - 1) >= 2^L"""
    return (h - 1) * 2 ** L


def shapes_stream(h, L):
    # fwd: even nr, nc % 4 == 0, nc >= 64, nr >= 2 hlen; inv: even nci >= 32, nri >= 2 hlen -- at every level
    return [(2 ** (L + 1) * h, 32 * 2 ** L)]


def shapes_lds(h, L):
    # fwd: nr >= 16, nr >= hp, nc >= hp; inv: nri >= hp, nci >= 2 (hp = the padded length) -- at every level; any parity
    n = max(16, 2 * pad8(h)) * 2 ** (L - 1)
    return [(n, n + 4), (n + 1, n + 3)]


def shapes_any(h, L):
    # no gate but the level clamp; any parity
    n = max(_clamp_side(h, L), 8 * 2 ** L)
    n += n & 1
    return [(n, n + 6), (n + 1, n + 3)]


def shapes_1d(h, L):
    # dwt1d_fused.hip: Nc >= 64; a power of two and an odd length; 9 rows (more than the 8 a workgroup of the row kernels packs)
    n = max(64, _clamp_side(h, L))
    p = 64
    while p < n:
        p *= 2
    return [(9, p), (9, n + 1 if not (n & 1) else n)]


def shapes_swt_fused(h, L, H=None):
    # swt_fused*.inc: Nc % 4 == 0, Nc >= 64, Nr % 2^(L-1) == 0, Nr / 2^(L-1) >= 2 H (H = the instantiated length), halo <= Nc
    H = H or h
    f = 2 ** (L - 1)
    nr = max(2 * H * f, _clamp_side(h, L))
    nr = -(-nr // f) * f
    nc = max(64, (_clamp_side(h, L) + 8 + 3) // 4 * 4)
    return [(nr, nc)]


def shapes_swt_twopass(h, L):
    # the fused shape (rows-in-LDS and ring kernels for banks of up to 20 taps) and an odd one (the direct kernels)
    m = max(h - 1, 2)
    return shapes_swt_fused(h, L, pad_l2(h) if h > 20 else h) + [(2 ** L * m + 1, max(2 ** L * m + 3, 67))]


def shapes_swt1d(h, L):
    n = max(64, (_clamp_side(h, L) + 4 + 3) // 4 * 4)
    return [(6, n), (3, max(_clamp_side(h, L) + 3, 67) | 1)]


# ---- evidence --------------------------------------------------------------------------------------------------------------------
FWD2D = ["fwd2d_fused", "fwd2d_casc", "fwd2d_stream", "fwd2d_f64", "ana_rows", "ana_cols"]
INV2D = ["inv2d_fused", "inv2d_casc", "inv2d_stream", "inv2d_f64", "syn_cols", "syn_rows"]
INV_CASC_STATS = ["stat_inv_casc3", "stat_inv_cascw", "stat_inv_casc2"]


def _only(all_names, ran):
    return list(ran), [n for n in all_names if n not in ran]


def ev_level(fwd, inv):
    def f(row, h, L, shape, direction):
        return _only(FWD2D, fwd) if direction == "fwd" else _only(INV2D, inv)
    return f


def ev_casc(stat):
    def f(row, h, L, shape, direction):
        # L = 3: the forward runs the pair and one level kernel; the inverse forms without a three-level launch for this length too
        level = ["fwd2d_stream", "fwd2d_f64"] if direction == "fwd" else ["inv2d_stream", "inv2d_f64"]
        if direction == "fwd":
            ran, quiet = _only(FWD2D, ["fwd2d_casc"])
        else:
            ran, quiet = _only(INV2D + INV_CASC_STATS, ["inv2d_casc", stat])
        three_in_one = direction == "inv" and (stat == "stat_inv_casc3" or (stat == "stat_inv_cascw" and h <= 12))
        if L == 3 and not three_in_one:  # (18 / 20 taps: that level is below the size floor of dwt_lds.hip and runs the tiled kernel)
            quiet = [n for n in quiet if n not in level + ["fwd2d_fused", "inv2d_fused"]]
        return ran, quiet
    return f


def ev_tiled_long(row, h, L, shape, direction):
    # 28 .. 34 taps, float32: the forward tile is over the LDS budget (two-pass), the inverse tile is not
    if direction == "inv":
        return _only(INV2D, ["inv2d_fused"])
    ran, quiet = _only(FWD2D, ["ana_rows", "ana_cols"])
    (ran if h in FAMILY_LENGTHS["PDWT_RING_HLENS"] else quiet).append("stat_ana_cols_ring")
    return ran, quiet + ["stat_ana_rows_tr"]


def ev_twopass(row, h, L, shape, direction):
    """names ending in @f32 / @f64 hold for that precision only"""
    ring = h in FAMILY_LENGTHS["PDWT_RING_HLENS"] and row["knobs"].get("tiled_cols", 0) != 1
    # rows_tr.hip: double precision only, knob rows_tr, Nc >= 2 hlen (analysis) / Nci >= hlen (synthesis) -- true at level 1 of every shape
    tr = row["knobs"].get("rows_tr", 1) == 1 and h in FAMILY_LENGTHS["PDWT_ROWS_TR_HLENS"]
    d = "ana" if direction == "fwd" else "syn"
    ran, quiet = _only(FWD2D if direction == "fwd" else INV2D, ["%s_rows" % d, "%s_cols" % d])
    (ran if ring else quiet).append("stat_%s_cols_ring" % d)
    (ran if tr else quiet).append("stat_%s_rows_tr@f64" % d)
    quiet.append("stat_%s_rows_tr@f32" % d)
    return ran, quiet


def ev_1d(fused):
    def f(row, h, L, shape, direction):
        d = "fwd" if direction == "fwd" else "inv"
        names = ["stat_%s1d_fused" % d, "stat_%s1d_fused_ip" % d]
        timer = "ana_rows" if direction == "fwd" else "syn_rows"
        if fused == "ip":
            return [timer, names[1]], [names[0]]
        if fused:
            return [timer, names[0]], [names[1]]
        tr = h in FAMILY_LENGTHS["PDWT_ROWS_TR_HLENS"]
        st = "stat_ana_rows_tr" if direction == "fwd" else "stat_syn_rows_tr"
        return [timer] + ([st + "@f64"] if tr else []), names + [st + "@f32"] + ([] if tr else [st + "@f64"])
    return f


def ev_haar(two_d):
    def f(row, h, L, shape, direction):
        k = ("haar2d_" if two_d else "haar1d_") + ("fwd" if direction == "fwd" else "inv")
        return [k], (FWD2D if direction == "fwd" else INV2D)
    return f


def ev_swt_fused(fam):
    def f(row, h, L, shape, direction):
        if direction == "fwd":
            ran, quiet = ["swt_ana_cols", "stat_%s_fwd" % fam], ["swt_ana_rows"] + [s for s in ("stat_swtf_fwd", "stat_swtl2_fwd", "stat_swtd_fwd") if s != "stat_%s_fwd" % fam]
        else:
            ran, quiet = ["swt_syn_cols", "stat_%s_inv" % fam], ["swt_syn_rows"] + [s for s in ("stat_swtf_inv", "stat_swtl2_inv", "stat_swtd_inv") if s != "stat_%s_inv" % fam]
            if fam == "swtf":  # tap spacing 4 (level 3) runs the residue-major kernel for the lengths it is instantiated for
                p = row["knobs"].get("swtf_perm", 1) == 1 and L >= 3 and h in FAMILY_LENGTHS["PDWT_SWTF_HLENS:3"]
                (ran if p else quiet).append("stat_swtf_invp")
            else:
                quiet.append("stat_swtf_invp")
        return ran, quiet
    return f


def ev_swt_twopass(row, h, L, shape, direction):
    d = "ana" if direction == "fwd" else "syn"
    ran = ["swt_%s_rows" % d, "swt_%s_cols" % d]
    quiet = ["stat_swtf_fwd", "stat_swtl2_fwd", "stat_swtd_fwd"] if direction == "fwd" else ["stat_swtf_inv", "stat_swtf_invp", "stat_swtl2_inv", "stat_swtd_inv"]
    fast = h <= 20 and shape[1] % 4 == 0 and shape[0] % 2 ** (L - 1) == 0  # (k_swt_rows_lds: Nc % 4 (2 in double); ring: Nr % fct, Nr / fct >= hlen)
    if fast:
        ran += ["stat_swt_%s_rows_lds" % d, "stat_swt_%s_cols_ring" % d]
    elif h > 20:
        quiet += ["stat_swt_%s_rows_lds" % d, "stat_swt_%s_cols_ring" % d]
    elif shape[1] % 2:  # an odd row length never passes the Nc % NV gate of k_swt_rows_lds: the direct row kernels
        quiet += ["stat_swt_%s_rows_lds" % d]
    return ran, quiet


def ev_swt1d(row, h, L, shape, direction):
    d = "ana" if direction == "fwd" else "syn"
    ran, quiet = ["swt_%s_rows" % d], ["swt_%s_cols" % d]
    if h <= 20 and shape[1] % 4 == 0:
        ran.append("stat_swt_%s_rows_lds" % d)
    elif h > 20 or shape[1] % 2:  # (an odd row length never passes the Nc % NV gate of k_swt_rows_lds)
        quiet.append("stat_swt_%s_rows_lds" % d)
    return ran, quiet


# ---- the rows --------------------------------------------------------------------------------------------------------------------
def _row(rid, kind, dtypes, knobs, accepts, shapes, evidence, inst, levels=1, levels2=2, banks=None, pad_check=None, pad_evidence=None):
    return dict(id=rid, kind=kind, dtypes=tuple(dtypes), knobs=knobs, accepts=accepts, shapes=shapes, evidence=evidence, inst=inst, levels=levels,
                levels2=levels2, banks=banks, pad_check=pad_check, pad_evidence=pad_evidence)


def E(template, key, mapping, ran, quiet=()):
    """one kernel template a bank of the row may run on: the template's name, the list it is instantiated from and the mapping of a
    bank length onto it, and the proof -- the name that must be in the case's `ran` evidence and the names that must be in its `quiet`
    evidence (the other kernels behind the same timer) for the case to count as a run of this template"""
    return dict(template=template, key=key, mapping=mapping, ran=ran, quiet=tuple(quiet))


def _both(fwd, inv):
    return dict(fwd=fwd, inv=inv)


def _twopass_inst(d, a, rows_alternates=()):
    """row kernel + column kernel of the two-pass / per-level forms; d = "ana" | "syn" """
    return [E("k_%s_rows" % d, "PDWT_TILED_HLENS", "generic", "%s_rows" % d, ("stat_%s_rows_tr" % d,) + tuple(rows_alternates)),
            E("k_%s_rows_tr" % d, "PDWT_ROWS_TR_HLENS", "exact", "stat_%s_rows_tr" % d)] + \
           ([E("k_%s_cols" % d, "PDWT_TILED_HLENS", "generic", "%s_cols" % d, ("stat_%s_cols_ring" % d,)),
             E("k_%s_cols_ring" % d, "PDWT_RING_HLENS", "exact", "stat_%s_cols_ring" % d)] if a else [])


_TWOPASS = _both(_twopass_inst("ana", True), _twopass_inst("syn", True))
_ROWS1D = _both(_twopass_inst("ana", False, ("stat_fwd1d_fused", "stat_fwd1d_fused_ip")), _twopass_inst("syn", False, ("stat_inv1d_fused", "stat_inv1d_fused_ip")))
_NOFAST = dict(stream=0, casc=0, f64_lds=0, f64_lat=0)


def _casc_inst(template, key, stat):
    return _both([E("k_fwd2d_casc", "PDWT_CASC_FWD_HLENS", "exact", "fwd2d_casc")], [E(template, key, "exact", stat)])


def pad_ev_lds(row, h, dt, direction):
    """knob f64_lds = 3 (exact lengths only): what runs a bank whose length is no multiple of 8 instead of dwt_lds.hip"""
    inverse = direction == "inv"
    fused = dt == F32 and tiled_fused_takes(h, 4, inverse)
    if not inverse:
        return (["fwd2d_fused"] if fused else ["ana_rows", "ana_cols"]), ["fwd2d_f64"]
    return (["inv2d_fused"] if fused else ["syn_cols", "syn_rows"]), ["inv2d_f64"]


def pad_ev_swt_long(row, h, dt, direction):
    d = "ana" if direction == "fwd" else "syn"
    return ["swt_%s_rows" % d, "swt_%s_cols" % d], ["stat_swtl2_%s" % direction]


def ev_one_buffer_inverse_only(row, h, L, shape, direction):
    # 22 .. 40 taps at 8192 doubles: the forward one-buffer kernel is not instantiated (per-level row kernels), the inverse one is
    if direction == "fwd":
        tr = h in FAMILY_LENGTHS["PDWT_ROWS_TR_HLENS"]
        return ["ana_rows"] + (["stat_ana_rows_tr"] if tr else []), ["stat_fwd1d_fused", "stat_fwd1d_fused_ip"] + ([] if tr else ["stat_ana_rows_tr"])
    return ["syn_rows", "stat_inv1d_fused_ip"], ["stat_inv1d_fused", "stat_syn_rows_tr"]


_SWTF = "PDWT_SWTF_HLENS:"
ROWS = [
    # ---- decimated 2-D ----
    _row("stream", "dwt2", [F32], dict(casc=0), lambda h: 4 <= h <= 16, shapes_stream, ev_level(["fwd2d_stream"], ["inv2d_stream"]),
         _both([E("k_fwd2d_stream", "PDWT_STREAM_FWD_HLENS", "exact", "fwd2d_stream")], [E("k_inv2d_stream", "PDWT_STREAM_INV_HLENS", "exact", "inv2d_stream")])),
    _row("casc_inv3", "dwt2", [F32], dict(casc_min=0, casc_iwaves=CASC_IWAVES), lambda h: h in (4, 8, 12, 16, 20), lambda h, L: [casc_shape("inv3", h)], ev_casc("stat_inv_casc3"),
         _casc_inst("k_inv2d_casc3", "inv2d_casc3_f32", "stat_inv_casc3"), levels=2, levels2=3),
    _row("casc_invw", "dwt2", [F32], dict(casc_min=0, casc_l3=2, casc_iwaves=CASC_IWAVES), lambda h: 4 <= h <= 18, lambda h, L: [casc_shape("invw", h)], ev_casc("stat_inv_cascw"),
         _casc_inst("k_inv2d_cascw", "PDWT_CASCW_INV_HLENS", "stat_inv_cascw"), levels=2, levels2=3),
    _row("casc_inv2", "dwt2", [F32], dict(casc_min=0, casc_iwg=1), lambda h: 4 <= h <= 10, lambda h, L: [casc_shape("inv2", h)], ev_casc("stat_inv_casc2"),
         _casc_inst("k_inv2d_casc", "PDWT_CASC_INV_HLENS", "stat_inv_casc2"), levels=2, levels2=3),
    _row("lds", "dwt2", [F32, F64], dict(f64_lds_min=0, stream=0, casc=0, f64_lat=0), lambda h: 4 <= h <= 40, shapes_lds, ev_level(["fwd2d_f64"], ["inv2d_f64"]),
         _both([E("k_fwd2d_f64lds", "PDWT_F64LDS_HLENS", "pad8", "fwd2d_f64")], [E("k_inv2d_f64lds", "PDWT_F64LDS_HLENS", "pad8", "inv2d_f64")]),
         pad_check=("f64_lds", 3), pad_evidence=pad_ev_lds),
    _row("lat", "dwt2", [F64], dict(f64_lat_min=256), lambda h: h == 40, lambda h, L: [(256 * 2 ** (L - 1), 256 * 2 ** (L - 1))],
         lambda row, h, L, shape, d: (["fwd2d_f64", "stat_lat_fwd"], [n for n in FWD2D if n != "fwd2d_f64"]) if d == "fwd"
         else (["inv2d_f64", "stat_lat_inv"], [n for n in INV2D if n != "inv2d_f64"]),
         _both([E("k_fwd2d_lat", "PDWT_LAT_HLENS", "exact", "stat_lat_fwd")], [E("k_inv2d_lat", "PDWT_LAT_HLENS", "exact", "stat_lat_inv")]), banks=["db20"]),
    _row("tiled", "dwt2", [F32], _NOFAST, lambda h: 4 <= h <= 26, shapes_any, ev_level(["fwd2d_fused"], ["inv2d_fused"]),
         _both([E("k_fwd2d_fused", "PDWT_TILED_HLENS", "generic", "fwd2d_fused")], [E("k_inv2d_fused", "PDWT_TILED_HLENS", "generic", "inv2d_fused")])),
    _row("tiled_long", "dwt2", [F32], _NOFAST, lambda h: 28 <= h <= 34, shapes_any, ev_tiled_long,
         _both(_TWOPASS["fwd"], [E("k_inv2d_fused", "PDWT_TILED_HLENS", "generic", "inv2d_fused")])),
    _row("twopass", "dwt2", [F32, F64], dict(force_twopass=1, rows_tr=1), lambda h: 4 <= h <= 40, shapes_any, ev_twopass, _TWOPASS),
    _row("twopass_tr0", "dwt2", [F64], dict(force_twopass=1, rows_tr=0), lambda h: h in (20, 24, 30, 40), shapes_any, ev_twopass, _TWOPASS),
    # (knob tiled_cols = 1 keeps the column pass off the ring kernels: the only way to k_ana_cols / k_syn_cols at the lengths the ring
    #  kernels are instantiated for)
    _row("twopass_tiled_cols", "dwt2", [F32, F64], dict(force_twopass=1, tiled_cols=1), lambda h: h in FAMILY_LENGTHS["PDWT_RING_HLENS"], shapes_any, ev_twopass, _TWOPASS),
    _row("haar2d", "dwt2", [F32, F64], dict(), lambda h: h == 2, lambda h, L: [(16 * 2 ** L, 16 * 2 ** L + 4 * 2 ** L), (37, 51)], ev_haar(True), _both([], []),
         levels=2, levels2=3, banks=["haar"]),
    # ---- batched 1-D ----
    _row("dwt1d_fused", "dwt1", [F32, F64], dict(), lambda h: 4 <= h <= 40, shapes_1d, ev_1d(True),
         _both([E("k_fwd1d_fused", "PDWT_1D_HLENS", "exact", "stat_fwd1d_fused")], [E("k_inv1d_fused", "PDWT_1D_HLENS", "exact", "stat_inv1d_fused")]), levels=2, levels2=3),
    # (rows of 8192 doubles are over the LDS budget of the two-buffer kernels; the one-buffer inverse keeps at most 2 x 256 16-byte chunks
    #  of A_L in registers -- inv_cap_x<2>(0) -- so A_L has at most 1024 samples: three levels or more at this length.  The forward
    #  one-buffer kernel is instantiated up to 20 taps, the inverse one for every length: the second row is the inverse alone)
    _row("dwt1d_one_buffer", "dwt1", [F64], dict(), lambda h: 4 <= h <= 20, lambda h, L: [(8, 8192)], ev_1d("ip"),
         _both([E("k_fwd1d_fused_ip", "PDWT_1D_HLENS", "exact", "stat_fwd1d_fused_ip")], [E("k_inv1d_fused_ip", "PDWT_1D_HLENS", "exact", "stat_inv1d_fused_ip")]),
         levels=3, levels2=4, banks="per_length"),
    _row("dwt1d_one_buffer_inv", "dwt1", [F64], dict(), lambda h: 22 <= h <= 40, lambda h, L: [(8, 8192)], ev_one_buffer_inverse_only,
         _both(_ROWS1D["fwd"], [E("k_inv1d_fused_ip", "PDWT_1D_HLENS", "exact", "stat_inv1d_fused_ip")]), levels=3, levels2=4, banks="per_length"),
    _row("dwt1d_rows", "dwt1", [F32, F64], dict(force_twopass=1), lambda h: 4 <= h <= 40, shapes_1d, ev_1d(False), _ROWS1D, levels=2, levels2=3),
    _row("haar1d", "dwt1", [F32, F64], dict(), lambda h: h == 2, lambda h, L: [(4, 64), (3, 77)], ev_haar(False), _both([], []), levels=2, levels2=3, banks=["haar"]),
    # ---- stationary 2-D ----
    _row("swt_fused", "swt2", [F32], dict(), lambda h: 2 <= h <= 20, shapes_swt_fused, ev_swt_fused("swtf"),
         _both([E("k_swt_fwd_fused", _SWTF + "1", "exact", "stat_swtf_fwd"), E("k_swt_fwd_fused", _SWTF + "4", "exact", "stat_swtf_fwd")],
               [E("k_swt_inv_fused4", _SWTF + "1", "exact", "stat_swtf_inv"), E("k_swt_inv_fused4", _SWTF + "4", "exact", "stat_swtf_inv"),
                E("k_swt_inv_fusedp", _SWTF + "3", "exact", "stat_swtf_invp")]), levels=3, levels2=2),
    _row("swt_fused_noperm", "swt2", [F32], dict(swtf_perm=0), lambda h: 8 <= h <= 16, shapes_swt_fused, ev_swt_fused("swtf"),
         _both([E("k_swt_fwd_fused", _SWTF + "1", "exact", "stat_swtf_fwd")], [E("k_swt_inv_fused4", _SWTF + "1", "exact", "stat_swtf_inv", ("stat_swtf_invp",))]),
         levels=3, levels2=2),
    _row("swt_fused_long", "swt2", [F32], dict(), lambda h: 22 <= h <= 40, lambda h, L: shapes_swt_fused(h, L, pad_l2(h)), ev_swt_fused("swtl2"),
         _both([E("k_swt_fwd_fused2", "PDWT_SWTL2_HLENS", "pad_l2", "stat_swtl2_fwd")], [E("k_swt_inv_fused2", "PDWT_SWTL2_HLENS", "pad_l2", "stat_swtl2_inv")]),
         levels=3, levels2=2, pad_check=("swtf_long", 0), pad_evidence=pad_ev_swt_long),
    _row("swt_fused_f64", "swt2", [F64], dict(), lambda h: 2 <= h <= 16, shapes_swt_fused, ev_swt_fused("swtd"),
         _both([E("k_swt_fwd_fused_d", "PDWT_SWTD_HLENS", "exact", "stat_swtd_fwd")], [E("k_swt_inv_fused_d", "PDWT_SWTD_HLENS", "exact", "stat_swtd_inv")]), levels=3, levels2=2),
    _row("swt_twopass", "swt2", [F32, F64], dict(swtf=0), lambda h: 2 <= h <= 40, shapes_swt_twopass, ev_swt_twopass,
         _both([E("k_swt_rows_lds_ana", "PDWT_SWT_ROWS_HLENS", "exact", "stat_swt_ana_rows_lds"), E("k_swt_ana_cols_ring", "PDWT_SWT_RING_HLENS", "exact", "stat_swt_ana_cols_ring")],
               [E("k_swt_rows_lds_syn", "PDWT_SWT_ROWS_HLENS", "exact", "stat_swt_syn_rows_lds"), E("k_swt_syn_cols_ring", "PDWT_SWT_RING_HLENS", "exact", "stat_swt_syn_cols_ring")]),
         levels=3, levels2=2),
    # ---- stationary 1-D ----
    _row("swt1d", "swt1", [F32, F64], dict(), lambda h: 2 <= h <= 40, shapes_swt1d, ev_swt1d,
         _both([E("k_swt_rows_lds_ana", "PDWT_SWT_ROWS_HLENS", "exact", "stat_swt_ana_rows_lds")], [E("k_swt_rows_lds_syn", "PDWT_SWT_ROWS_HLENS", "exact", "stat_swt_syn_rows_lds")]),
         levels=3, levels2=2),
]

# ---- the kernel templates and the instantiations of each that a transform can reach: {template: {precision: lengths}}, 0 = the
# run-time-length form (H = 0) of the templates that have one.  The closing test of tests/test_all_banks_gpu.py wants every entry run
# and proved by launch evidence; tests/test_bank_matrix_cpu.py checks that the cases can do that.
_T = FAMILY_LENGTHS


def _templates():
    both, f32, f64 = ("float32", "float64"), ("float32",), ("float64",)
    swtf = _T[_SWTF + "1"] + _T[_SWTF + "4"]
    t = {}

    def add(names, lens, dts):
        for n in names:
            t[n] = {d: sorted(lens) for d in dts}
    add(["k_fwd2d_stream"], _T["PDWT_STREAM_FWD_HLENS"], f32)
    add(["k_inv2d_stream"], _T["PDWT_STREAM_INV_HLENS"], f32)
    add(["k_fwd2d_casc"], _T["PDWT_CASC_FWD_HLENS"], f32)
    add(["k_inv2d_casc3"], _T["inv2d_casc3_f32"], f32)
    add(["k_inv2d_cascw"], _T["PDWT_CASCW_INV_HLENS"], f32)
    add(["k_inv2d_casc"], _T["PDWT_CASC_INV_HLENS"], f32)
    add(["k_fwd2d_f64lds", "k_inv2d_f64lds"], _T["PDWT_F64LDS_HLENS"], both)
    add(["k_fwd2d_lat", "k_inv2d_lat"], _T["PDWT_LAT_HLENS"], f64)
    # the tiled fused kernels: float32 only and only while the tile fits the LDS budget (never in double precision, see above)
    add(["k_fwd2d_fused"], [0] + [h for h in _T["PDWT_TILED_HLENS"] if tiled_fused_takes(h, 4, False)], f32)
    add(["k_inv2d_fused"], [0] + [h for h in _T["PDWT_TILED_HLENS"] if tiled_fused_takes(h, 4, True)], f32)
    add(["k_ana_rows", "k_syn_rows", "k_ana_cols", "k_syn_cols"], [0] + _T["PDWT_TILED_HLENS"], both)
    add(["k_ana_rows_tr", "k_syn_rows_tr"], _T["PDWT_ROWS_TR_HLENS"], f64)
    add(["k_ana_cols_ring", "k_syn_cols_ring"], _T["PDWT_RING_HLENS"], both)
    add(["k_fwd1d_fused", "k_inv1d_fused"], _T["PDWT_1D_HLENS"], both)
    add(["k_fwd1d_fused_ip"], [h for h in _T["PDWT_1D_HLENS"] if h <= 20], f64)  # (dwt1d_fused.hip: `HLEN <= 20`)
    add(["k_inv1d_fused_ip"], _T["PDWT_1D_HLENS"], f64)
    add(["k_swt_rows_lds_ana", "k_swt_rows_lds_syn"], _T["PDWT_SWT_ROWS_HLENS"], both)
    add(["k_swt_ana_cols_ring", "k_swt_syn_cols_ring"], _T["PDWT_SWT_RING_HLENS"], both)
    add(["k_swt_fwd_fused", "k_swt_inv_fused4"], swtf, f32)
    add(["k_swt_inv_fusedp"], _T[_SWTF + "3"], f32)
    add(["k_swt_fwd_fused2", "k_swt_inv_fused2"], _T["PDWT_SWTL2_HLENS"], f32)
    add(["k_swt_fwd_fused_d", "k_swt_inv_fused_d"], _T["PDWT_SWTD_HLENS"], f64)
    return t


TEMPLATES = _templates()
EXPECTED_REACH = {(t, d, n) for t, per in TEMPLATES.items() for d, lens in per.items() for n in lens}


def resolve(names, dt):
    """evidence names of one precision: `name@f32` / `name@f64` hold for that precision only"""
    sfx = "@f32" if dt == F32 else "@f64"
    return [n.split("@")[0] for n in names if "@" not in n or n.endswith(sfx)]


def case_reaches(row, wname, dt, shape, L):
    """{(template, precision, instantiated length)} that a PASSED case of the row proves to have run: the template's proof name is in the
    evidence the case asserts as `ran` and the other kernels behind the same timer are in what it asserts as `quiet`"""
    h, out = hlen_of(wname), set()
    for d in ("fwd", "inv"):
        ran, quiet = row["evidence"](row, h, L, shape, d)
        ran, quiet = resolve(ran, dt), resolve(quiet, dt)
        for e in row["inst"][d]:
            t = instantiation(e["key"], e["mapping"], h)
            if t is not None and e["ran"] in ran and all(q in quiet for q in e["quiet"]):
                out.add((e["template"], dt.name, t))
    return out


ROW_BY_ID = {r["id"]: r for r in ROWS}
PER_LENGTH = one_bank_per_length()


def row_banks(row):
    banks = PER_LENGTH if row["banks"] == "per_length" else (row["banks"] or ALL72)
    return [b for b in banks if row["accepts"](hlen_of(b))]


def row_cases(row, levels=None):
    """[(bank, shape, L)] of the all-banks sweep of a row (levels = None) or of its second level count (one bank per length)"""
    L = row["levels"] if levels is None else levels
    banks = row_banks(row) if levels is None else [b for b in row_banks(row) if b in PER_LENGTH]
    return [(b, s, L) for b in banks for s in row["shapes"](hlen_of(b), L)]


def case_input(wname, shape):
    """uniform(-100, 100), one seed per bank, rounded to float32: both precisions, every family and the reference see the same values"""
    return np.random.RandomState(2000 + ALL72.index(wname)).uniform(-100, 100, shape).astype(np.float32)
