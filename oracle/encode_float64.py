"""FLOAT64 EVALUATOR of the encoding's five linear maps.  TEST INFRASTRUCTURE ONLY (imported by ``tests/`` alone).

The encoding is piecewise linear: once the simplex of a (point, level) is fixed, the forward is a gather and every gradient a
gather or a scatter with known coefficients.  A float64 re-evaluation OF THE SIMPLEX is no reference (at a fine level the
elevated coordinate is ~1e5 with an fp32 ulp of 8e-3: float64 lands in another simplex), so what the kernels compute bit for
bit -- ``rem0``, ``rank``, the table rows ``idx[N, P+1]`` and the fp32 barycentrics ``bary[N, P+1]`` -- is taken from the fp32
restatement (``permuto_oracle.simplex`` / ``vertex_indices``, unchanged; they also run on GPU tensors), and everything after
it is float64 here, without autograd.  The Jacobian ``J[n, r, k] = d bary_r / d pos_k`` is exact given ``rank``:

    dE[i][k] = sf[k] * ( 1 if k+1 > i,  -i if k+1 == i,  else 0 )          i = 0..P, k = 0..P-1
    for i in 0..P:  d = dE[i] / (P+1);  J[:, P - rank_i] += d;  J[:, P+1 - rank_i] -= d
    J[:, 0] += J[:, P+1]

Every map returns three tensors of one shape: the float64 VALUE, the SUM OF THE ABSOLUTE VALUES of its finest-grain terms
and the NUMBER of those terms ``m``, entry by entry.  A finest-grain term is a single product without a cancelling sum inside
(``w bary lat``; ``w bary g``; ``w g lat sf_k c / (P+1)`` for one (vertex slot, elevated coordinate) pair; ...), so that an fp32
evaluation in ANY summation order errs by at most ``(m - 1 + r) u sum|t|``, r = roundings spent on forming one term.
``error_bar`` below is that bound; the callers state r.

Layouts: features / upstream gradients ``[N, C]`` (channel ``l * F + f``, then the concatenated-point channels of
``permuto_oracle.nr_point_channels``), tables ``[L, T, F]``; the term counts of a table are per row, ``[L, T, 1]``.
"""
import torch

from . import permuto_oracle as po

U = 2.0 ** -24            # unit roundoff of fp32
TINY = 2.0 ** -126        # smallest normal fp32: a term that underflows (or is flushed) errs by at most this


def error_bar(sum_abs, m, r):
    """|fp32 result - float64 value| <= (m + r) u sum|t| + m 2^-126, entry by entry.  r: roundings on the longest path that
    forms one term (counted from the kernel's expressions by the caller); the m - 1 additions in any order are the rest."""
    m = m.to(torch.float64)
    return (m + float(r)) * U * sum_abs + m * TINY


def jacobian(rank, sf):
    """rank [N, P+1] int64, sf [P] -> (J, sum|terms|, number of non-zero terms), each [N, P+1, P] float64.
    The terms of J[n, r, k] are the products sf_k c / (P+1), one per elevated coordinate i that feeds slot r."""
    N, P1 = rank.shape
    P = P1 - 1
    dev = rank.device
    sf = torch.as_tensor(sf).to(dev).double()
    dE = torch.zeros(P + 1, P, dtype=torch.float64, device=dev)
    for i in range(P + 1):
        for k in range(P):
            dE[i, k] = (1.0 if k + 1 > i else (-float(i) if k + 1 == i else 0.0)) * sf[k]
    J = torch.zeros(N, P + 2, P, dtype=torch.float64, device=dev)
    A = torch.zeros_like(J)
    C = torch.zeros_like(J)
    rows = torch.arange(N, device=dev)
    for i in range(P + 1):
        d = dE[i] / (P + 1)
        nz = (d != 0).double()
        up, dn = P - rank[:, i], P + 1 - rank[:, i]
        J[rows, up] += d
        J[rows, dn] -= d
        A[rows, up] += d.abs()
        A[rows, dn] += d.abs()
        C[rows, up] += nz
        C[rows, dn] += nz
    for X in (J, A, C):
        X[:, 0] += X[:, P + 1]
    return J[:, :P + 1], A[:, :P + 1], C[:, :P + 1]


def scatter_rows(rows, vals, nr_rows):
    """out[rows[i]] += vals[i] in float64 WITHOUT atomics (a coarse level sends a whole batch to a handful of rows: float64
    atomics on one address serialise for seconds): sort by row, then sum every row's run by itself, in two passes (runs are cut
    into pieces of 1024 so that a crowded row does not become one long serial sum).  A row's error is relative to ITS OWN terms:
    a running sum over the whole sorted batch with differences at the row boundaries -- the first form of this helper -- errs by
    2^-53 x the prefix, which swamps a row whose only contribution has a barycentric weight of 1e-10 behind a prefix of 100.
    rows [M] int64, vals [M, K] float64 -> [nr_rows, K]."""
    out = torch.zeros(nr_rows, vals.shape[1], dtype=torch.float64, device=vals.device)
    M = rows.numel()
    if M == 0:
        return out
    order = torch.argsort(rows)
    v = vals[order].contiguous()
    uniq, inv, counts = torch.unique_consecutive(rows[order], return_inverse=True, return_counts=True)
    starts = counts.cumsum(0) - counts
    pos = torch.arange(M, device=rows.device) - starts[inv]
    key = inv * ((M >> 10) + 1) + (pos >> 10)                          # non-decreasing: (row, piece of its run)
    _, piece_len = torch.unique_consecutive(key, return_counts=True)
    part = torch.segment_reduce(v, "sum", lengths=piece_len, axis=0, unsafe=True)
    seg = torch.segment_reduce(part, "sum", lengths=(counts + 1023) >> 10, axis=0, unsafe=True)
    out[uniq] = seg
    return out


class Encoding64:
    """One batch of points against one set of parameters.  points [N, P] fp32, lattice [L, T, F] fp32, sf [L, P] fp32
    (``permuto_oracle.scale_factors`` or the product's ``scale_factor`` tensor: same values), shifts [L, P] fp32, window [L]
    fp32, concat_mode 0 / 1 (padded pseudo-levels) / 2 (exactly P channels), all on one device."""

    def __init__(self, points, lattice, sf, shifts, window, concat_mode=0, points_scaling=1.0, cache=True):
        self.pts = points.detach()
        self.lat = lattice.detach()
        self.dev = points.device
        self.N, self.P = points.shape
        self.L, self.T, self.F = lattice.shape
        self.sf = sf.detach().to(self.dev)
        self.shifts = shifts.detach().to(self.dev)
        self.win = window.detach().to(self.dev)
        self.w64 = [float(v) for v in self.win.double().cpu()]
        self.mode = int(concat_mode)
        self.npc = {0: 0, 1: self.F * po.nr_extra_levels(self.P, self.F, True), 2: self.P}[self.mode]
        self.C = self.L * self.F + self.npc
        self.ps = float(torch.tensor(points_scaling, dtype=torch.float32).double())     # the kernels take it as an fp32 argument
        self._cache = {} if cache else None

    def level(self, l):
        """-> idx [N, P+1] int64, bary [N, P+1] float64 (the fp32 values), J, |J| terms, J term counts [N, P+1, P]"""
        if self._cache is not None and l in self._cache:
            return self._cache[l]
        with torch.no_grad():
            rem0, rank, bary = po.simplex(self.pts, self.shifts[l], self.sf[l])
            idx = po.vertex_indices(rem0, rank, self.T)
            out = (idx, bary[:, :self.P + 1].double()) + jacobian(rank, self.sf[l])
        if self._cache is not None:
            self._cache[l] = out
        return out

    def open_levels(self):
        return [l for l in range(self.L) if self.w64[l] != 0.0]

    def _zeros(self, *shape):
        return [torch.zeros(*shape, dtype=torch.float64, device=self.dev) for _ in range(3)]

    # -------------------------------------------------------------------------------------------------- forward
    def forward(self):
        """feat[n, l, f] = w_l sum_r bary_r lat[l, idx_r, f]; concatenated channels points_scaling * pos."""
        F = self.F
        val, mag, cnt = self._zeros(self.N, self.C)
        for l in self.open_levels():
            idx, bary, _, _, _ = self.level(l)
            lat = self.lat[l].double()
            for r in range(self.P + 1):
                t = lat[idx[:, r]] * (bary[:, r:r + 1] * self.w64[l])
                val[:, l * F:(l + 1) * F] += t
                mag[:, l * F:(l + 1) * F] += t.abs()
            cnt[:, l * F:(l + 1) * F] = self.P + 1
        if self.npc:
            c0 = self.L * F
            t = self.pts.double() * self.ps
            val[:, c0:c0 + self.P] = t
            mag[:, c0:c0 + self.P] = t.abs()
            cnt[:, c0:c0 + self.P] = 1
        return val, mag, cnt

    # ------------------------------------------------------------------------------------------ lattice gradient
    def lattice_grad(self, g):
        """gl[l, idx_r, f] += w_l bary_r g[n, l, f]; counts [L, T, 1] = contributions per row."""
        F = self.F
        val, mag = self._zeros(self.L, self.T, F)[:2]
        cnt = torch.zeros(self.L, self.T, 1, dtype=torch.float64, device=self.dev)
        g = g.double()
        for l in self.open_levels():
            idx, bary, _, _, _ = self.level(l)
            gl = g[:, l * F:(l + 1) * F] * self.w64[l]
            rows = idx.t().reshape(-1)
            t = torch.cat([gl * bary[:, r:r + 1] for r in range(self.P + 1)], 0)
            s = scatter_rows(rows, torch.cat([t, t.abs()], 1), self.T)
            val[l], mag[l] = s[:, :F], s[:, F:]
            cnt[l, :, 0] = torch.bincount(rows, minlength=self.T).double()
        return val, mag, cnt

    # ----------------------------------------------------------------------------------------- position gradient
    def position_grad(self, g):
        """gp[n, k] = sum_l w_l sum_r sum_f g[n, l, f] lat[l, idx_r, f] J[n, r, k]  +  points_scaling g of the concatenated
        channels.  Terms: one product per (level, feature, vertex slot, elevated coordinate)."""
        F, P = self.F, self.P
        val, mag, cnt = self._zeros(self.N, P)
        g = g.double()
        for l in self.open_levels():
            idx, _, J, A, Cn = self.level(l)
            lat = self.lat[l].double()
            gl = g[:, l * F:(l + 1) * F] * self.w64[l]
            for r in range(P + 1):
                lv = lat[idx[:, r]] * gl                                  # [N, F]
                val += lv.sum(1, keepdim=True) * J[:, r]
                mag += lv.abs().sum(1, keepdim=True) * A[:, r]
                cnt += F * Cn[:, r]
        if self.npc:
            c0 = self.L * F
            t = g[:, c0:c0 + P] * self.ps
            val += t
            mag += t.abs()
            cnt += 1
        return val, mag, cnt

    # ------------------------------------------------------------------------------------------- double backward
    def _q(self, l, u):
        """q[n, r] = J[n, r, :] . u_n with its term magnitudes and counts, [N, P+1] each"""
        _, _, J, A, Cn = self.level(l)
        u = u.double()[:, None, :]
        return (J * u).sum(2), (A * u.abs()).sum(2), Cn.sum(2)

    def double_backward_gathered(self, u):
        """gg[n, l, f] = w_l sum_r (J[n, r, :] . u_n) lat[l, idx_r, f]; concatenated channels points_scaling * u."""
        F = self.F
        val, mag, cnt = self._zeros(self.N, self.C)
        for l in self.open_levels():
            idx = self.level(l)[0]
            q, qa, qc = self._q(l, u)
            lat = self.lat[l].double()
            for r in range(self.P + 1):
                lv = lat[idx[:, r]] * self.w64[l]
                val[:, l * F:(l + 1) * F] += lv * q[:, r:r + 1]
                mag[:, l * F:(l + 1) * F] += lv.abs() * qa[:, r:r + 1]
                cnt[:, l * F:(l + 1) * F] += qc[:, r:r + 1]
        if self.npc:
            c0 = self.L * F
            t = u.double() * self.ps
            val[:, c0:c0 + self.P] = t
            mag[:, c0:c0 + self.P] = t.abs()
            cnt[:, c0:c0 + self.P] = 1
        return val, mag, cnt

    def double_backward_scattered(self, u, g, g2=None):
        """gl[l, idx_r, f] += w_l (J[n, r, :] . u_n) g[n, l, f]  (+ w_l bary_r g2[n, l, f]: the plain scatter of a direct
        gradient riding along); counts [L, T, 1] = finest-grain terms per row."""
        F = self.F
        val, mag = self._zeros(self.L, self.T, F)[:2]
        cnt = torch.zeros(self.L, self.T, 1, dtype=torch.float64, device=self.dev)
        g = g.double()
        g2 = None if g2 is None else g2.double()
        for l in self.open_levels():
            idx, bary = self.level(l)[:2]
            q, qa, qc = self._q(l, u)
            gl = g[:, l * F:(l + 1) * F] * self.w64[l]
            rows = idx.t().reshape(-1)
            t = torch.cat([gl * q[:, r:r + 1] for r in range(self.P + 1)], 0)
            a = torch.cat([gl.abs() * qa[:, r:r + 1] for r in range(self.P + 1)], 0)
            c = torch.cat([qc[:, r:r + 1] for r in range(self.P + 1)], 0)
            if g2 is not None:
                g2l = g2[:, l * F:(l + 1) * F] * self.w64[l]
                t2 = torch.cat([g2l * bary[:, r:r + 1] for r in range(self.P + 1)], 0)
                t, a, c = t + t2, a + t2.abs(), c + 1
            s = scatter_rows(rows, torch.cat([t, a, c], 1), self.T)
            val[l], mag[l], cnt[l] = s[:, :F], s[:, F:2 * F], s[:, 2 * F:]
        return val, mag, cnt
