"""Test-side oracle of ROI coding: oracle.mlic_ref_cpu.RefMLIC with the VBR gain as a plane.

The reference's VBR slice loop (RefMLIC._slice_loop with `scale`) restated with a gain per latent pixel in place
of the scalar: y_hat = round((y - mu) * g) * (1 / g) + mu, the table index from sigma * g, the likelihood at
(y, sigma, mu) * g.  A map cell is 4 latent pixels wide and the checkerboard squeeze keeps every other column, so
the squeezed plane of either phase is g[..., ::2].  Plain torch on the CPU; reads nothing outside the repository.
"""
import torch

import mlic_ref_cpu as ref


def expand_levels(levels, gains):
    """levels integer [B,hz,wz], gains fp32 [n] -> the gain plane fp32 [B,1,4 hz,4 wz] (nearest expansion)."""
    g = torch.as_tensor(gains, dtype=torch.float32)[torch.as_tensor(levels).long()]
    return g.repeat_interleave(4, 1).repeat_interleave(4, 2).unsqueeze(1).contiguous()


class RefMLICRoi(ref.RefMLIC):
    def _slice_loop_g(self, hyper, g, y=None, record=None, collect_lik=True):
        """RefMLIC._slice_loop (encoder / forward side) with the plane g [B,1,H,W] in place of `scale`."""
        cfg = self.cfg
        S, C = cfg.slice_num, cfg.slice_ch
        hyper_means = hyper[:, cfg.hyper_M:]
        table = ref.scale_table()
        assert g.shape == (hyper.shape[0], 1, hyper.shape[2], hyper.shape[3]) and g.dtype == torch.float32
        rg = 1.0 / g
        g_sq = g[..., ::2]  # the squeezed plane of either phase (cells are 4 latent pixels wide)
        assert torch.equal(g_sq, g[..., 1::2])
        yh, liks = [], []

        def phase(anchor, y_part, s_part, m_part, ph):
            if record is not None:
                s_sq = ref.ckbd_squeeze(s_part, anchor)
                m_sq = ref.ckbd_squeeze(m_part, anchor)
                y_sq = ref.ckbd_squeeze(y_part, anchor)
                idx = ref.build_indexes(s_sq * g_sq, table)
                record(ph, torch.round((y_sq - m_sq) * g_sq).int(), idx)
            return torch.round((y_part - m_part) * g) * rg + m_part

        for idx in range(S):
            y_slice = y[:, idx * C:(idx + 1) * C]
            ya, yn = ref.ckbd_anchor(y_slice), ref.ckbd_nonanchor(y_slice)
            if idx == 0:
                pa = self.entropy_parameters(hyper, "anchor", idx)
            else:
                prev = torch.cat(yh, dim=1)
                inter = self.inter_context(prev, idx)
                chan = self.channel_context(prev, idx)
                pa = self.entropy_parameters(torch.cat([inter, chan, hyper], dim=1), "anchor", idx)
            sa, ma = pa.chunk(2, 1)
            sa, ma = ref.ckbd_anchor(sa), ref.ckbd_anchor(ma)
            anc = phase(True, ya, sa, ma, 2 * idx)
            anc = anc + ref.ckbd_anchor(self.lrp(torch.cat([hyper_means] + yh + [anc], dim=1), "anchor", idx))
            local = self.local_context(anc, idx)
            if idx == 0:
                pn = self.entropy_parameters(torch.cat([local, hyper], dim=1), "nonanchor", idx)
            else:
                intra = self.intra_context(yh[-1], anc, idx)
                pn = self.entropy_parameters(torch.cat([local, intra, inter, chan, hyper], dim=1), "nonanchor", idx)
            sn, mn = pn.chunk(2, 1)
            sn, mn = ref.ckbd_nonanchor(sn), ref.ckbd_nonanchor(mn)
            if collect_lik:
                s_all, m_all = sa + sn, ma + mn
                liks.append(ref.gaussian_likelihood(y_slice * g, s_all * g, m_all * g))
            non = phase(False, yn, sn, mn, 2 * idx + 1)
            cur = anc + non
            cur = cur + ref.ckbd_nonanchor(self.lrp(torch.cat([hyper_means] + yh + [cur], dim=1), "nonanchor", idx))
            yh.append(cur)
        return torch.cat(yh, dim=1), (torch.cat(liks, dim=1) if liks else None)

    @torch.no_grad()
    def forward_g(self, x, g, record=None):
        """RefMLIC.forward with the plane; record(phase, symbols, indexes) also receives the coder lists of
        RefMLIC.compress_streams (the same pass: forward and compress quantise alike)."""
        y = self.g_a(x)
        z = self.h_a(y)
        z_lik = self.eb_likelihood(z)
        med = self.eb_medians()
        z_hat = torch.round(z - med) + med
        hyper = self.h_s(z_hat)
        y_hat, y_lik = self._slice_loop_g(hyper, g, y=y, record=record)
        return {"x_hat": self.g_s(y_hat), "likelihoods": {"y_likelihoods": y_lik, "z_likelihoods": z_lik},
                "y_hat": y_hat}
