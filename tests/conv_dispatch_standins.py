"""Recording stand-ins for the launch wrappers `hip_ops.conv3x3` chooses between (tests/test_conv_partial_host.py, tests/halo_host_surface_common.py):
no launch of the library from a host test."""
import torch

from tests import fake_kernels


class Launches:
    """`log`: which wrapper was called, as the dispatch tests assert it.  `detail`: the same calls with every routing argument as received."""

    def __init__(self, monkeypatch, K):
        fake_kernels.install(monkeypatch)
        self.log, self.detail = [], []
        monkeypatch.setattr(K, "conv3x3_supported", lambda x, w, stride, padding: True)
        monkeypatch.setattr(K, "PARTIAL_CONV_RULES", False)                  # (the mechanics: every shape of a routed kind; the measured rule has its own test)
        monkeypatch.setattr(K, "CONV_HALO_MIN_TILES", 1)
        monkeypatch.setattr(K, "gn_emit_ok", lambda *a: False)

        def out(x, w, ups):
            n, h, wd, _ = x.shape
            return torch.zeros(n, 2 * h if ups else h, 2 * wd if ups else wd, w.shape[0], dtype=x.dtype, device=x.device)

        def tagged(y, emit_gn):
            return (y, torch.zeros(1)) if emit_gn else y

        def halo(x, w, bias=None, temb=None, res=None, temb_div=1, upsample=False, x2_nhwc=None, gn_coef=None, gn_act=True, emit_gn=False, shortcut=None,
                 partial_tiles=False):
            kind = "halo_sc" if shortcut is not None else "halo"
            self.log.append((kind, partial_tiles))
            self.detail.append((kind, bool(partial_tiles), bool(emit_gn), bool(upsample), temb is not None, res is not None))
            return tagged(out(x, w, upsample), emit_gn)

        def halo4(x, w, bias=None, temb=None, res=None, temb_div=1, upsample=False, x2_nhwc=None, emit_gn=False, split_k=None, wide=False,
                  partial_tiles=False, tw=None):
            self.log.append(("halo4", partial_tiles, tw))
            self.detail.append(("halo4", bool(partial_tiles), bool(emit_gn), bool(upsample), temb is not None, res is not None, tw, split_k, bool(wide)))
            return tagged(out(x, w, upsample), emit_gn)

        def upfold(x, w, bias=None, emit_gn=False, arm=None, partial_tiles=False, tw=None):
            self.log.append(("upfold", arm))
            self.detail.append(("upfold", bool(partial_tiles), bool(emit_gn), arm, tw))
            return tagged(out(x, w, True), emit_gn)

        def ring(x, w, bias=None, temb=None, res=None, tile=0, temb_div=1, upsample=False, stride2=False, **kw):
            self.log.append(("ring",))
            self.detail.append(("ring", bool(upsample), bool(stride2)))
            n, h, wd, _ = x.shape
            h, wd = (2 * h, 2 * wd) if upsample else ((h // 2, wd // 2) if stride2 else (h, wd))
            return torch.zeros(n, h, wd, w.shape[0], dtype=x.dtype, device=x.device)
        for name, fn in (("conv3x3_halo", halo), ("conv3x3_halo4", halo4), ("conv3x3_upfold", upfold), ("conv3x3_bf16", ring)):
            monkeypatch.setattr(K, name, fn)
        monkeypatch.setattr(K, "_pick", lambda *a, **kw: 1)

    def take(self):
        log, self.log, self.detail = self.log, [], []
        return log

    def take_detail(self):
        detail, self.log, self.detail = self.detail, [], []
        return detail
