"""A NumPy / Python restatement of dft_ldos::update and dft_ldos::ldos (src/dft_ldos.cpp:60-166),
the yardstick of the LDOS tests.  It is driven by whole-cell field arrays taken after every step
(the oracle's, or a run that steps one step per call) and sums in the reference's order, one
term after the other.

points: (comp[n], ijk[n, 3], amp[n]) in list order, the first nE of them the electric sources'
points.  get_array(c) -> the whole-cell array of component c (indexed by the global indices of
the cell's dimensions)."""
import cmath
import math

import numpy as np

EPS53 = 2.0 ** -53


class LdosRef:
    def __init__(self, freqs, dt, a, dim):
        self.freq = [float(f) for f in freqs]
        self.dt, self.dim = float(dt), dim
        self.dV = (1.0 / a) ** dim  # gv.dV(icenter, 1).computational_volume()
        self.Fdft = [0j] * len(self.freq)
        self.Jdft = [0j] * len(self.freq)
        self.Jsum = 1.0
        self.saved_overall_scale = 1.0
        # for the accumulation bound: the sums of |term| of F and J, the updates, the most points
        self.abs_F = 0.0
        self.abs_J = 0.0
        self.updates = 0
        self.npoints = 0

    def _value(self, arr, ijk):
        if self.dim == 3:
            return float(arr[ijk[0], ijk[1], ijk[2]])
        if self.dim == 2:
            return float(arr[ijk[0], ijk[1]])
        return float(arr[ijk[2]])

    def update(self, t, get_array, points, nE, J):
        """One dft_ldos::update at step count t.  J: real(sources->current()) of the first
        source, or None when there is no source at all."""
        comp, ijk, amp = points
        arrays = {}
        EJ, HJ, Jsum, absterm = 0j, 0j, 0.0, 0.0
        for p in range(len(comp)):
            c = int(comp[p])
            if c not in arrays:
                arrays[c] = np.asarray(get_array(c))
            f = self._value(arrays[c], ijk[p])
            A = complex(amp[p])
            term = complex(f * A.real, f * -A.imag)  # double * conj(A)
            if p < nE:
                EJ += term
            else:
                HJ += term
            Jsum += abs(A)
            absterm += abs(f) * abs(A)
        scale = self.dt / math.sqrt(2 * math.pi)
        time = t * self.dt
        for i, f in enumerate(self.freq):
            Ephase = cmath.rect(1.0, 2 * math.pi * f * time) * scale
            Hphase = cmath.rect(1.0, 2 * math.pi * f * (time - self.dt / 2)) * scale
            self.Fdft[i] += Ephase * EJ + Hphase * HJ
            if J is not None:
                self.Jdft[i] += Ephase * J
        self.Jsum = Jsum * math.sqrt(self.dV)
        self.abs_F += scale * absterm
        self.abs_J += scale * abs(J or 0.0)
        self.updates += 1
        self.npoints = max(self.npoints, len(comp))

    def overall_scale(self):
        return 4.0 / math.pi * -0.5 / (self.Jsum * self.Jsum)

    def ldos(self):
        s = self.overall_scale()
        out = []
        for F, J in zip(self.Fdft, self.Jdft):
            abs2 = J.real * J.real + J.imag * J.imag
            if abs2 == 0.0:
                out.append(float("nan"))
            else:
                out.append(s * (F * J.conjugate()).real / abs2)
        return np.array(out)

    def F(self):
        return np.array(self.Fdft)

    def J(self):
        return np.array(self.Jdft)

    # the project's accumulation bound (N + U + 64) 2^-53 sum|term| over N points and U updates
    def tol_F(self):
        return (self.npoints + self.updates + 64) * EPS53 * self.abs_F

    def tol_J(self):
        return (1 + self.updates + 64) * EPS53 * self.abs_J

    def tol_ldos(self, F=None, J=None):
        """The bound of ldos that follows from tol_F and tol_J: s Re(F conj J) / |J|^2 moves by at
        most |s| (dF |J| + |F| dJ) / |J|^2 + 2 |ldos| dJ / |J| (first order), plus a few roundings
        of the formula itself."""
        F = self.F() if F is None else F
        J = self.J() if J is None else J
        s = abs(self.overall_scale())
        aJ = np.abs(J)
        ld = np.abs(self.ldos())
        dF, dJ = self.tol_F(), self.tol_J()
        return s * (dF * aJ + np.abs(F) * dJ) / aJ ** 2 + 2 * ld * dJ / aJ + 16 * EPS53 * (
            s * np.abs(F) / aJ)


def custom_current(func, t, dt, start=0.0, end=1e20):
    """real(current) of a non-integrated custom source as dft_ldos::update reads it at step count
    t: func at the time of the last calc_sources, (t - 1) dt + dt (src/step.cpp:106,
    src/meep.hpp:1066-1078); 0 before the first step."""
    if t == 0:
        return 0.0
    time = (t - 1) * dt + dt
    rt = float(np.float32(time))
    if not (rt >= start and rt <= end):
        return 0.0
    return complex(func(time)).real
