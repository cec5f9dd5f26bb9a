"""CPU checks of the mode-coefficient layer: the argument handling of
DiffractedPlanewave / add_mode_monitor / get_eigenmode_coefficients against a stub fields
object, the two C-ABI entries in the header and the ctypes table, and the host mode table
(meep_nl_amd/csrc/mnl_modes.hpp) built by a stand-alone program under the address and
undefined-behaviour sanitizers and compared with closed forms in NumPy.

u = 2^-53.  k and the amplitudes agree within 16 u relative (to the largest entry of the vector:
a component that vanishes by symmetry is not 0 to the last bit); a unit-modulus phase within
(|2 pi k dx| + 16) u absolute, which covers the rounding of the argument itself."""
import os
import re
import subprocess

import numpy as np
import pytest

import meep_nl_amd as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
NEW = ["mnl_fields_mode_coefficients", "mnl_fields_mode_table"]


# ------------------------------------------------------------------ Python layer
class StubFields:
    def __init__(self, nfreq):
        self.nfreq = nfreq
        self.calls = []

    def add_dft_flux(self, regs, freqs, decimation):
        self.added = (regs, list(freqs), decimation)
        return 3

    def mode_coefficients(self, h, modes, eig_vol=None, kpoint=None):
        self.calls.append((h, list(modes), eig_vol, kpoint))
        nm, nf = len(modes), self.nfreq
        kp = np.zeros(3) if kpoint is None else np.asarray(kpoint, dtype=float)
        alpha = np.zeros((nm, nf, 2), dtype=complex)
        for m in range(nm):
            for i in range(nf):
                alpha[m, i] = [m + 10 * i + kp[0], -1j * (m + 10 * i)]
        k = np.zeros((nm, nf, 3))
        k[..., 2] = 1.0 + np.arange(nf)[None, :] + kp[2]
        return {"alpha": alpha, "vgrp": np.full((nm, nf), 0.5), "kpoints": k,
                "cscale": np.full((nm, nf), 2.0), "overlaps": np.zeros((nm, nf, 8), dtype=complex)}


def stub_sim(nfreq):
    sim = mp.Simulation(cell_size=mp.Vector3(2, 2, 3), resolution=8)
    sim.fields = StubFields(nfreq)
    sim.init_sim = lambda: None  # the stub stands for initialised fields
    return sim


def test_diffracted_planewave_properties():
    dp = mp.DiffractedPlanewave((1, -1, 0), mp.Vector3(0, 1, 0), 1, 0.5j)
    assert tuple(dp.g) == (1, -1, 0) and dp.axis == mp.Vector3(0, 1, 0)
    assert dp.s == 1 + 0j and dp.p == 0.5j and isinstance(dp.s, complex)
    assert mp.DiffractedPlanewave((0, 0, 0), None, 1, 0).axis is None
    with pytest.raises(AttributeError):
        dp.g = (0, 0, 0)  # read-only, as python/simulation.py:191-205


def test_get_eigenmode_coefficients_argument_forms():
    sim = stub_sim(3)
    mon = sim.add_mode_monitor(0.5, 0.2, 3, mp.FluxRegion(center=mp.Vector3(z=0.5),
                                                          size=mp.Vector3(2, 2, 0)))
    assert isinstance(mon, mp.DftFlux) and mon.handle == 3 and mon in sim.dft_objects
    assert sim.fields.added[0][0][2] == 2  # the z normal
    one = mp.DiffractedPlanewave((1, 0, 0), None, 1, 0)
    res = sim.get_eigenmode_coefficients(mon, one, eig_parity=7)
    assert type(res).__name__ == "EigCoeffsResult" and res._fields == (
        "alpha", "vgrp", "kpoints", "kdom", "cscale")
    assert res.alpha.shape == (1, 3, 2) and res.alpha.dtype == np.complex128
    assert res.vgrp.shape == (3,) and res.cscale.shape == (3,)
    assert len(res.kpoints) == 3 and res.kdom[1] == mp.Vector3(0, 0, 2.0)
    h, modes, ev, kp = sim.fields.calls[-1]
    assert h == 3 and ev is None and kp is None
    assert tuple(modes[0][0]) == (1, 0, 0) and modes[0][1] is None and modes[0][2:] == (1, 0)
    # a list is one call
    two = [one, mp.DiffractedPlanewave((0, 1, 0), mp.Vector3(1, 0, 0), 0.5, 0.5j)]
    n = len(sim.fields.calls)
    res = sim.get_eigenmode_coefficients(mon, two, eig_vol=mp.Volume(mp.Vector3(0, 0, 0.5),
                                                                      size=mp.Vector3(1, 2, 0)))
    assert len(sim.fields.calls) == n + 1 and res.alpha.shape == (2, 3, 2)
    assert res.vgrp.shape == (6,) and len(res.kdom) == 6
    assert sim.fields.calls[-1][2] == ([-0.5, -1.0, 0.5], [0.5, 1.0, 0.5])
    assert res.alpha[1, 2, 0] == 21 and res.alpha[1, 2, 1] == -21j
    # kpoint_func: evaluated per (band, frequency); equal kpoints share a call
    seen = []

    def kf(freq, band):
        seen.append((freq, band))
        return mp.Vector3(0.25 if freq > 0.5 else 0.0, 0, 0.5)
    n = len(sim.fields.calls)
    res = sim.get_eigenmode_coefficients(mon, two, kpoint_func=kf)
    assert len(seen) == 6 and all(b == 1 for _, b in seen)
    assert len(sim.fields.calls) == n + 2
    assert res.alpha[0, 0, 0] == 0 and res.alpha[1, 2, 0] == 21.25
    assert res.kdom[5] == mp.Vector3(0, 0, 3.5)


def test_integer_bands_and_bad_arguments_raise():
    sim = stub_sim(1)
    mon = sim.add_mode_monitor([0.5], mp.FluxRegion(center=mp.Vector3(), size=mp.Vector3(2, 2, 0)))
    for bands in ([1], [1, 2], range(1, 3), 1):
        with pytest.raises(NotImplementedError, match="MPB"):
            sim.get_eigenmode_coefficients(mon, bands)
    with pytest.raises(TypeError, match="bands"):
        sim.get_eigenmode_coefficients(mon, "1")
    with pytest.raises(TypeError, match="bands"):
        sim.get_eigenmode_coefficients(mon, [])
    with pytest.raises(NotImplementedError, match="direction"):
        sim.get_eigenmode_coefficients(mon, mp.DiffractedPlanewave((0, 0, 0), None, 1, 0),
                                       direction=mp.X)
    sim.get_eigenmode_coefficients(mon, mp.DiffractedPlanewave((0, 0, 0), None, 1, 0),
                                   direction=mp.Z)
    sim.fields = None
    with pytest.raises(ValueError, match="initialized"):
        sim.get_eigenmode_coefficients(mon, mp.DiffractedPlanewave((0, 0, 0), None, 1, 0))


def test_header_declares_the_entry_points():
    txt = open(os.path.join(ROOT, "include", "meep_nl_amd.h")).read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))
    assert ("int mnl_fields_mode_coefficients(mnl_fields *f, int handle, int nmodes, const int *g, "
            "const double *axis, const double *sp, const double *eig_vol, const double *kpoint, "
            "double *coeffs, double *vgrp, double *kpoints, double *cscale, double *overlaps);"
            ) in flat
    assert ("int mnl_fields_mode_table(mnl_fields *f, int handle, int nmodes, const int *g, "
            "const double *axis, const double *sp, const double *eig_vol, const double *kpoint, "
            "long long *dims, int *coords, double *k, double *vgrp, double *amp, double *pa, "
            "double *pb, double *pl);") in flat
    assert "src/mpb.cpp:925-1004" in txt
    from meep_nl_amd import _lib
    for name in NEW:
        assert name in _lib.exported_symbols()
    assert len(_lib._SIGS["mnl_fields_mode_coefficients"][1]) == 13
    assert len(_lib._SIGS["mnl_fields_mode_table"][1]) == 16


# ------------------------------------------------------------------ the host table
@pytest.fixture(scope="module")
def table_output(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("modes") / "mode_table")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "meep_nl_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpu", "mode_table_main.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


def _fl(words):
    return [float.fromhex(w) for w in words]


def _cx(words):
    v = _fl(words)
    return np.array(v[0::2]) + 1j * np.array(v[1::2])


def parse(out):
    cases, errors, cur = {}, {}, None
    for line in out.splitlines():
        w = line.split()
        if w[0] == "error":
            errors[w[1]] = line.split("|", 1)[1].strip()
        elif w[0] == "case":
            cur = cases[w[1]] = {"modes": {}, "k": {}, "amp": {}, "pa": {}, "pb": {}, "pl": {}}
        elif w[0] == "geom":
            i = [int(x) for x in w[1:16]]
            f = _fl(w[16:])
            cur.update(has=i[0:3], ncell=i[3:6], periodic=i[6:9], normal=i[9], da=i[10], db=i[11],
                       nlayer=i[12], layer=i[13:15], bloch=f[0:3], a=f[3], emin=f[4:7],
                       emax=f[7:10], kpoint=f[10:13], eps=f[13], mu=f[14])
        elif w[0] in ("ca", "cb"):
            cur[w[0]] = [int(x) for x in w[1:]]
        elif w[0] == "freqs":
            cur["freqs"] = _fl(w[1:])
        elif w[0] == "mode":
            f = _fl(w[5:])
            cur["modes"][int(w[1])] = dict(g=[int(x) for x in w[2:5]], axis=f[0:3],
                                           s=complex(f[3], f[4]), p=complex(f[5], f[6]))
        elif w[0] in ("pa", "pb"):
            cur[w[0]][int(w[1])] = _cx(w[2:])
        elif w[0] == "k":
            cur["k"][(int(w[1]), int(w[2]))] = (int(w[3]), np.array(_fl(w[4:7])), float.fromhex(w[7]))
        elif w[0] in ("amp", "pl"):
            cur[w[0]][(int(w[1]), int(w[2]))] = _cx(w[3:])
    return cases, errors


def closed_form(c, m, f):
    """(evanescent, k, vgrp, E0, H0, in-plane k) of mode m at frequency f, from the issue's
    formulas (src/mpb.cpp:342-347, 619-664)."""
    M = c["modes"][m]
    n = c["normal"]
    ext = [c["emax"][d] - c["emin"][d] for d in range(3)]
    kp = list(c["kpoint"])
    for d in range(3):
        if not c["has"][d] or d == n:
            continue
        num = 1 if ext[d] == 0 else int(ext[d] * c["a"] + 0.5)
        if num == c["ncell"][d] and c["periodic"][d]:
            kp[d] = c["bloch"][d]
    k = np.array(kp, dtype=float)
    k2sum = 0.0
    for d in range(3):
        if c["has"][d] and ext[d] != 0:
            k[d] = kp[d] + M["g"][d] / ext[d]
            k2sum += k[d] * k[d]
    kin = k.copy()
    fr = c["freqs"][f]
    k2 = fr * fr * (c["eps"] * c["mu"]) - k2sum
    if k2 < 0:
        return True, np.zeros(3), 0.0, np.zeros(3), np.zeros(3), kin
    if k2 > 0:
        k[n] = np.sqrt(k2)
    ax = np.array(M["axis"], dtype=float)
    if not ax.any():
        ax[c["da"]] = 1.0
    sh = np.cross(ax, k)
    sh = sh / np.linalg.norm(sh)
    ph = np.cross(sh, k / np.linalg.norm(k))
    E0 = M["s"] * sh + M["p"] * ph
    H0 = np.cross(k, E0) / (fr * c["mu"])
    return False, k, k[n] / (fr * c["eps"] * c["mu"]), E0, H0, kin


def check_case(c):
    h = 0.5 / c["a"]
    cen = [0.5 * (c["emin"][d] + c["emax"][d]) for d in range(3)]
    n = c["normal"]
    for m in c["modes"]:
        for f in range(len(c["freqs"])):
            ev, k, vg, E0, H0, kin = closed_form(c, m, f)
            gev, gk, gvg = c["k"][(m, f)]
            amp = c["amp"][(m, f)]
            assert gev == int(ev), (m, f)
            if ev:  # all 0, as src/mpb.cpp:957-962
                assert not gk.any() and gvg == 0 and not amp.any()
                continue
            assert np.all(np.abs(gk - k) <= 16 * U * np.abs(k).max()), (m, f, gk, k)
            assert abs(gvg - vg) <= 16 * U * abs(vg), (m, f)
            for got, want in ((amp[:3], E0), (amp[3:], H0)):
                assert np.all(np.abs(got - want) <= 16 * U * np.abs(want).max()), (m, f, got, want)
            # transversality: the plane wave of the table is one
            assert abs(np.dot(k, amp[:3])) <= 64 * U * np.linalg.norm(k) * np.abs(amp[:3]).max()
            for l in range(c["nlayer"]):
                arg = 2 * np.pi * k[n] * (c["layer"][l] * h - cen[n])
                assert abs(c["pl"][(m, f)][l] - np.exp(1j * arg)) <= (abs(arg) + 16) * U, (m, f, l)
        _, _, _, _, _, kin = closed_form(c, m, len(c["freqs"]) - 1)
        for name, d, co in (("pa", c["da"], c["ca"]), ("pb", c["db"], c["cb"])):
            if d < 0:
                assert np.array_equal(c[name][m], [1.0])
                continue
            arg = 2 * np.pi * kin[d] * (np.array(co) * h - cen[d])
            assert np.all(np.abs(c[name][m] - np.exp(1j * arg)) <= (np.abs(arg) + 16) * U), (name, m)


def test_mode_table_against_closed_forms(table_output):
    cases, errors = parse(table_output)
    assert set(cases) == {"normal_incidence", "evanescent_to_propagating", "k2_zero", "bloch",
                          "bloch_short_volume", "image_coordinates", "normal_x", "normal_y",
                          "two_d"}
    for name, c in cases.items():
        check_case(c)
    assert "parallel to the wavevector" in errors["axis_parallel"]
    # what each case is there for
    c = cases["normal_incidence"]
    assert np.array_equal(c["k"][(0, 1)][1], [0, 0, 1.0]) and c["k"][(0, 1)][2] == 1.0
    assert np.all(c["pa"][0] == 1) and np.all(c["pb"][1] == 1)
    c = cases["evanescent_to_propagating"]
    assert [c["k"][(0, f)][0] for f in range(3)] == [1, 0, 0]
    assert c["k"][(0, 1)][1][0] == 0.5 and c["k"][(0, 1)][1][2] == np.sqrt(0.75 ** 2 - 0.25)
    c = cases["k2_zero"]  # k[n] stays at the caller's value
    assert c["k"][(0, 0)][0] == 0 and np.array_equal(c["k"][(0, 0)][1], [0.5, 0, 0.125])
    c = cases["bloch"]  # x: the Bloch k; y: spanned but not periodic, the caller's kpoint
    assert c["k"][(0, 0)][1][0] == 0.1 and c["k"][(0, 0)][1][1] == 0.05
    c = cases["bloch_short_volume"]  # shorter than the period: kpoint + g / extent
    assert c["k"][(0, 0)][1][0] == 0.3 + 1 / 1.0
    c = cases["image_coordinates"]
    assert c["ca"][0] == -19 and c["ca"][-1] == 19 and c["nlayer"] == 2
    assert cases["two_d"]["db"] == -1 and cases["normal_x"]["normal"] == 0
