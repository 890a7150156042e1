"""The host surface of the halo convolutions as data (tools/record_halo_host_surface.py writes it to tests/golden/halo_host_surface.json,
tests/test_halo_host_surface.py asserts that the tree reproduces the file): what every exported predicate and count function returns over a grid,
the (return code, message) of failing calls to the launch and pack entry points, and the launch `hip_ops.conv3x3` makes over the shipped sizes.
Nothing here launches: the failing calls are refused by their argument checks (pointers are made-up integers), the routes run on recording
stand-ins with storage-less tensors."""
import itertools
import json

import torch

from tests.conv_dispatch_standins import Launches

HS, WS = range(1, 22), range(1, 71)
CHANNELS = [(cin, cout) for cin in (64, 240, 320, 1280) for cout in (80, 200, 240, 320)]
N_IMGS = (2, 4096)                                   # 4096 images of 21 x 70 x 1280 channels: an operand past 2 GiB


def rle(seq):
    """[v, v, v, w, ...] -> [v, 3, w, 1, ...]"""
    runs = []
    for v in seq:
        if runs and runs[-2] == v:
            runs[-1] += 1
        else:
            runs += [v, 1]
    return runs


def unrle(runs):
    return [v for v, k in zip(runs[::2], runs[1::2]) for _ in range(k)]


def same_table(got, want, what, expand):
    """Equal tables, naming the first element that differs where they are not (`expand`: (table, value) -> the flat list a value stands for)."""
    got = json.loads(json.dumps(got))
    assert [r[:-1] for r in got["rows"]] == [r[:-1] for r in want["rows"]], f"{what}: the rows themselves differ"
    for g, w in zip(got["rows"], want["rows"]):
        a, b = expand(got, got["values"][g[-1]]), expand(want, want["values"][w[-1]])
        if a != b:
            at = next(i for i, (x, y) in enumerate(zip(a, b)) if x != y)
            raise AssertionError(f"{what} {g[:-1]}: element {at} is {a[at]}, recorded {b[at]}")
    assert got == want, what


class _Table:
    """Rows `[key..., index]` into a list of distinct values: most rows of a part share few values."""

    def __init__(self):
        self.values, self.rows, self._at = [], [], {}

    def index(self, value):
        h = repr(value)
        if h not in self._at:
            self._at[h] = len(self.values)
            self.values.append(value)
        return self._at[h]

    def add(self, key, value):
        self.rows.append(list(key) + [self.index(value)])

    def data(self):
        return {"values": self.values, "rows": self.rows}


# ---- 1. predicates and counts: one row per (function, arguments other than H and W).  Its value: over H in 1 .. 21, runs of image rows; an image row
# (`lines`): the results over W in 1 .. 70 as runs.  Functions are named by their index in `names` ----
def predicates(L):
    t, lines, names = _Table(), _Table(), []

    def plane(name, fn, *key):
        f = getattr(L, name)
        if name not in names:
            names.append(name)
        t.add((names.index(name),) + key, rle([lines.index(rle([int(fn(f, h, w)) for w in WS])) for h in HS]))

    plane("fmc_conv3x3_halo_tiles_per_image", lambda f, h, w: f(h, w))
    plane("fmc_conv3x3_halo_partial_tiles_per_image", lambda f, h, w: f(h, w))
    plane("fmc_conv3x3_halo4_row_blocks_per_image", lambda f, h, w: f(h, w))
    for wide in (0, 1):
        plane("fmc_conv3x3_halo4_partial_tw", lambda f, h, w: f(h, w, wide), wide)
    for tw in (8, 16):
        plane("fmc_conv3x3_halo4_partial_row_blocks_per_image", lambda f, h, w: f(h, w, tw), tw)
    for n, (cin, cout) in itertools.product(N_IMGS, CHANNELS):
        for p in ("", "_partial"):
            for ups in (0, 1):
                plane(f"fmc_conv3x3_halo{p}_supported", lambda f, h, w: f(n, h, w, cin, cin, cout, ups), n, cin, cout, ups)
                for wide in (0, 1):
                    plane(f"fmc_conv3x3_halo4{p}_supported", lambda f, h, w: f(n, h, w, cin, cin, cout, ups, wide), n, cin, cout, ups, wide)
            # (the shortcut of a block with Cout channels: one source of cin channels, or [cin | cin])
            for cin_sc in (cin, 2 * cin):
                plane(f"fmc_conv3x3_halo_sc{p}_supported", lambda f, h, w: f(n, h, w, cout, cout, cin_sc, cin), n, cin, cout, cin_sc)
            plane(f"fmc_conv3x3_halo_fold{p}_supported", lambda f, h, w: f(n, h, w, cin, cout), n, cin, cout)
            for wide in (0, 1):
                plane(f"fmc_conv3x3_halo4_fold{p}_supported", lambda f, h, w: f(n, h, w, cin, cout, wide), n, cin, cout, wide)
    for n, cout, wide in itertools.product(N_IMGS, (80, 200, 240, 320), (0, 1)):
        plane("fmc_conv3x3_halo4_tiles", lambda f, h, w: f(n, h, w, cout, wide), n, cout, wide)
        for tw in (8, 16):
            plane("fmc_conv3x3_halo4_partial_tiles", lambda f, h, w: f(n, h, w, cout, wide, tw), n, cout, wide, tw)
    return dict(t.data(), lines=lines.values, names=names)


def expand_plane(data, value):
    """A value of `predicates` as the flat list over (H, W)."""
    return [v for line in unrle(value) for v in unrle(data["lines"][line])]


# ---- 2. errors: failing calls of the ten launch and four pack entry points.  Every row breaks at least one argument check, so none reaches its launch ----
X, X2, WP, BIAS, TEMB, RES, OUT, GN, WSP, XS, XS2, COEF = (0x10000 * k for k in range(1, 13))
FULL = ("x", "x2", "Cin1", "w", "bias", "temb", "res", "out", "n", "H", "W", "Cin", "Cout", "temb_ld", "temb_div", "ups")
SIGS = {
    "fmc_conv3x3_halo_bf16": FULL + ("gn_coef", "gn_act", "gn_part", "stream"),
    "fmc_conv3x3_halo_sc_bf16": ("x", "w", "bias", "temb", "out", "xs", "xs2", "Cin_sc1", "Cin_sc", "n", "H", "W", "Cin", "Cout", "temb_ld", "temb_div",
                                 "gn_part", "stream"),
    "fmc_conv3x3_halo_fold_bf16": ("x", "w", "bias", "out", "n", "H", "W", "Cin", "Cout", "gn_part", "stream"),
    "fmc_conv3x3_halo4_bf16": FULL + ("gn_part", "split_k", "ws", "ws_bytes", "wide", "stream"),
    "fmc_conv3x3_halo4_fold_bf16": ("x", "w", "bias", "out", "n", "H", "W", "Cin", "Cout", "gn_part", "wide", "stream"),
}
SIGS["fmc_conv3x3_halo_partial_bf16"] = SIGS["fmc_conv3x3_halo_bf16"]
SIGS["fmc_conv3x3_halo_sc_partial_bf16"] = SIGS["fmc_conv3x3_halo_sc_bf16"]
SIGS["fmc_conv3x3_halo_fold_partial_bf16"] = SIGS["fmc_conv3x3_halo_fold_bf16"]
SIGS["fmc_conv3x3_halo4_partial_bf16"] = SIGS["fmc_conv3x3_halo4_bf16"][:-1] + ("tw", "stream")
SIGS["fmc_conv3x3_halo4_fold_partial_bf16"] = SIGS["fmc_conv3x3_halo4_fold_bf16"][:-1] + ("tw", "stream")
BASE = dict(x=X, x2=None, Cin1=320, w=WP, bias=BIAS + 8, temb=None, res=None, out=OUT, n=2, H=11, W=64, Cin=320, Cout=320, temb_ld=0, temb_div=1, ups=0,
            gn_coef=None, gn_act=0, gn_part=None, stream=None, xs=XS, xs2=None, Cin_sc1=320, Cin_sc=320, split_k=1, ws=None, ws_bytes=0, wide=0, tw=16)
WS_BYTES = lambda split, a: split * a["n"] * a["H"] * a["W"] * a["Cout"] * 4


def error_calls():
    """[(entry point, label, arguments)]"""
    rows = []

    def row(name, label, **over):
        a = dict(BASE, **over)
        rows.append((name, label, [a[k] for k in SIGS[name]]))

    for name, sig in SIGS.items():
        partial, full, c4, sc = "_partial" in name, "temb" in sig, "halo4" in name, "_sc_" in name
        for k in ("x", "w", "out"):
            row(name, f"null {k}", **{k: None})
            row(name, f"misaligned {k}", **{k: BASE[k] + 8})
        row(name, "misaligned bias", bias=BIAS + 4)
        row(name, "null x, refused shape", x=None, Cin=96)                      # (the order of the checks: NULL first ...)
        row(name, "refused shape, misaligned x", x=X + 8, Cout=200)             # (... the shape before the alignment)
        # refused shapes at a whole width and at ragged ones (the partial entry points refuse the second for its channels alone)
        row(name, "channels, whole width", Cin=96, Cin1=96)
        row(name, "channels out, whole width", Cout=200)
        row(name, "ragged width 44", W=44, **({"Cout": 200} if partial else {}))
        row(name, "ragged width 7", W=7, **({"Cin": 96, "Cin1": 96} if partial else {}))
        row(name, "no image", n=0)
        row(name, "width 0", W=0)
        row(name, "operand of 2 GiB", n=4096, H=512, W=512)
        for cout in (160, 1920):                                               # statistics: Cout % 64, the channel tile % (Cout / 32)
            row(name, f"statistics at Cout {cout}", gn_part=GN, Cout=cout)
        row(name, "misaligned out, statistics at Cout 160", out=OUT + 8, gn_part=GN, Cout=160)
        if full:
            row(name, "misaligned temb", temb=TEMB + 4, temb_ld=320)
            row(name, "temb row stride", temb=TEMB, temb_ld=322)
            for div in (0, -3):
                row(name, f"temb_img_div {div}", temb=TEMB, temb_ld=320, temb_div=div)
            row(name, "misaligned bias, temb_img_div 0", bias=BIAS + 2, temb=TEMB, temb_ld=320, temb_div=0)
            row(name, "temb_img_div 0, statistics at Cout 160", temb=TEMB, temb_ld=160, temb_div=0, gn_part=GN, Cout=160)
        if full and not sc:
            row(name, "misaligned x2", x2=X2 + 8, Cin1=256, Cin=320)
            row(name, "misaligned residual", res=RES + 4)
            row(name, "first source's channels", x2=X2, Cin1=96)
            row(name, "first source past all", x2=X2, Cin1=384)
            row(name, "upsample of an odd size", ups=1, H=11)
        if sc:
            row(name, "null shortcut input", xs=None)
            row(name, "misaligned shortcut input", xs=XS + 8)
            row(name, "misaligned second shortcut input", xs2=XS2 + 8, Cin_sc=640)
            row(name, "shortcut channels", Cin_sc=96, Cin_sc1=96)
            row(name, "second shortcut source's channels", xs2=XS2, Cin_sc=416, Cin_sc1=320)
            row(name, "null shortcut input, misaligned x", xs=None, x=X + 8)   # (the conv's own checks come first)
        if c4:
            row(name, "wide, Cout % 160", wide=1, Cout=240)
            row(name, "wide at width 24", wide=1, W=24, **({"Cout": 240} if partial else {}))
            if partial:
                for tw, wide in ((4, 0), (0, 0), (32, 0), (8, 1)):
                    row(name, f"tw {tw} wide {wide}", tw=tw, wide=wide)
                row(name, "tw 12 at width 12", tw=12, W=12)
        if c4 and full:
            for split in (2, 5, 99):
                a = dict(BASE)
                need = WS_BYTES(min(split, 5), a)
                row(name, f"split_k {split} with statistics", split_k=split, gn_part=GN, ws=WSP, ws_bytes=need)
                row(name, f"split_k {split} without workspace", split_k=split)
                row(name, f"split_k {split}, short workspace", split_k=split, ws=WSP, ws_bytes=need - 1)
                row(name, f"split_k {split}, misaligned workspace", split_k=split, ws=WSP + 8, ws_bytes=need)
            row(name, "split_k 2 at ragged width 44, short workspace", split_k=2, W=44 if partial else 40, ws=WSP, ws_bytes=100)
    P4 = ("w", "dst", "Cin", "Cout")
    packs = {"fmc_conv3x3_halo_pack_weight": P4 + ("stream",), "fmc_conv3x3_halo4_pack_weight": P4 + ("wide", "stream"),
             "fmc_conv3x3_upfold_pack_weight": P4 + ("tile", "stream"), "fmc_conv3x3_halo_sc_pack_weight": ("w", "wsc", "dst", "Cin", "Cout", "Cin_sc", "tile", "stream")}
    pbase = dict(w=X, wsc=X2, dst=OUT, Cin=320, Cout=320, Cin_sc=640, wide=0, tile=160, stream=None)
    for name, sig in packs.items():
        def prow(label, **over):
            a = dict(pbase, **over)
            rows.append((name, label, [a[k] for k in sig]))
        for k in sig:
            if k in ("w", "wsc", "dst"):
                prow(f"null {k}", **{k: None})
                prow(f"misaligned {k}", **{k: pbase[k] + 8})
        prow("Cin % 64", Cin=96)
        prow("Cout % tile", Cout=200)
        prow("null w, Cin % 64", w=None, Cin=96)
        prow("Cin % 64, misaligned dst", Cin=96, dst=OUT + 4)
        if "tile" in sig:
            prow("tile 96", tile=96)
            prow("tile 80, Cout 200", tile=80, Cout=200)
        if "wide" in sig:
            prow("wide, Cout 240", wide=1, Cout=240)
        if "Cin_sc" in sig:
            prow("Cin_sc % 64", Cin_sc=96)
            prow("Cin_sc 0", Cin_sc=0)
            prow("Cin 0", Cin=0)
    return rows


REFUSALS = (-1, -3, -5)                             # FMC_E_SHAPE, FMC_E_ALIGN, FMC_E_NULL: the argument checks' codes (FMC_E_LAUNCH = -4 would be a launch)


def errors(L):
    """Rows `[entry point (index in `names`), label, index]`, values `[return code, message]`."""
    t, names = _Table(), []
    for name, label, args in error_calls():
        rc = int(getattr(L, name)(*args))
        msg = L.fmc_last_error()
        if name not in names:
            names.append(name)
        t.add((names.index(name), label), [rc, msg.decode() if msg else ""])
    return dict(t.data(), names=names)


# ---- 3. routes: the launch `hip_ops.conv3x3` makes, and `shortcut_fold_ok`, over the shipped sizes ----
# (n, H, W) of the input: the shipped sizes, and two at which conv_halo4 leaves statistics (H W >= GN_MIN_HW, one workgroup per tile; whole and ragged)
SIZES = ((32, 40, 64), (32, 20, 32), (32, 10, 16), (32, 5, 8), (16, 32, 48), (16, 16, 24), (16, 8, 12), (16, 4, 6), (4, 8, 48), (4, 7, 7),
         (4, 64, 40), (2, 64, 36))
ROUTE_CHANNELS = [(cin, cout) for cin in (320, 640, 1280, 1920) for cout in (320, 640, 1280, 240, 200)]
# the operands and modes of a call: (upsample, stride 2, temb, residual, emit_gn, grad enabled)
CALLS = {"plain": (0, 0, 0, 0, 0, 0), "upsample": (1, 0, 0, 0, 0, 0), "upsample+gn": (1, 0, 0, 0, 1, 0), "upsample+temb": (1, 0, 1, 0, 0, 0),
         "upsample+grad": (1, 0, 0, 0, 0, 1), "stride2": (0, 1, 0, 0, 0, 0), "temb": (0, 0, 1, 0, 0, 0), "residual": (0, 0, 0, 1, 0, 0),
         "temb+residual+gn": (0, 0, 1, 1, 1, 0), "gn": (0, 0, 0, 0, 1, 0), "grad": (0, 0, 0, 0, 0, 1), "gn+grad": (0, 0, 0, 0, 1, 1)}
# the switches: PARTIAL_TILES, PARTIAL_CONV_RULES, CONV_HALO_MIN_TILES, and one of CONV_HALO4 / UPS_FOLD / SHORTCUT_FOLD off
SWITCHES = [dict(PARTIAL_TILES=pt, PARTIAL_CONV_RULES=rules, CONV_HALO_MIN_TILES=mt) for pt in (False, True) for rules in (True, False) for mt in (1, 200)]
SWITCHES += [dict(PARTIAL_TILES=True, PARTIAL_CONV_RULES=False, CONV_HALO_MIN_TILES=1, **{off: False}) for off in ("CONV_HALO4", "UPS_FOLD", "SHORTCUT_FOLD")]
ALL_KINDS = frozenset(("halo", "halo_sc", "halo4", "upfold_halo", "upfold_halo4"))


class _OnDevice(torch.Tensor):
    """A storage-less tensor that says it lives on the GPU: what `shortcut_fold_ok` asks of its operands, on a host without one."""
    is_cuda = property(lambda self: True)


def image(*shape, nchw=False, cuda=False):
    t = torch.empty(*shape, dtype=torch.bfloat16, device="meta")
    if cuda:
        t = t.as_subclass(_OnDevice)
    return t.permute(0, 3, 1, 2) if nchw else t


def filter_cl(cout, cin):
    return torch.empty(cout, cin, 3, 3, dtype=torch.bfloat16, device="meta").contiguous(memory_format=torch.channels_last)


def routes(K, monkeypatch):
    """Rows `[switch set (index in `switches`), call, index]`: the value holds, per (size, channels) in order, what the stand-ins received, as runs.  Shortcut rows: per
    (size, channels, one / two shortcut sources) `[shortcut_fold_ok, launch]`.  With every kind routed and with the default ones."""
    default_kinds, switches = K.PARTIAL_CONV_ROUTED, []
    calls = Launches(monkeypatch, K)
    t = _Table()
    launches, at = [], {}                              # (distinct launches, so that a run holds an index)

    def launch_id(detail):
        if repr(detail) not in at:
            at[repr(detail)] = len(launches)
            launches.append(detail)
        return at[repr(detail)]

    for sw, kinds in itertools.product(SWITCHES, (ALL_KINDS, None)):
        if kinds is None and not sw["PARTIAL_TILES"]:
            continue                                    # (the routed kinds matter with the switch on alone)
        for k, v in {**dict(CONV_HALO4=True, UPS_FOLD=True, SHORTCUT_FOLD=True, PARTIAL_CONV_ROUTED=default_kinds if kinds is None else kinds), **sw}.items():
            monkeypatch.setattr(K, k, v)
        switches.append([sorted(sw.items()), "all kinds" if kinds is not None else "default kinds"])
        key = [len(switches) - 1]
        for call, (ups, s2, temb, res, gn, grad) in CALLS.items():
            seq = []
            for (n, h, w), (cin, cout) in itertools.product(SIZES, ROUTE_CHANNELS):
                ho, wo = (2 * h, 2 * w) if ups else ((h // 2, w // 2) if s2 else (h, w))
                with torch.set_grad_enabled(bool(grad)):
                    K.conv3x3(image(n, h, w, cin, nchw=True), filter_cl(cout, cin), None, image(n // 4, cout) if temb else None,
                              image(n, ho, wo, cout, nchw=True) if res else None, stride=(2, 2) if s2 else (1, 1), temb_div=4, upsample=bool(ups), emit_gn=bool(gn))
                seq.append(launch_id(calls.take_detail()))
            t.add(key + [call], rle(seq))
        seq = []
        for (n, h, w), (cin, cout), two in itertools.product(SIZES, ROUTE_CHANNELS, (False, True)):
            x, wt = image(n, h, w, cout, nchw=True, cuda=True), filter_cl(cout, cout)
            xs = image(n, h, w, cin, nchw=True, cuda=True)
            with torch.no_grad():
                ok = bool(K.shortcut_fold_ok(x, wt, xs, xs if two else None))
                if ok:
                    K.conv3x3(x, wt, None, emit_gn=True, shortcut=(xs, xs if two else None, image(cout, (2 if two else 1) * cin), None))
            seq.append(launch_id([ok] + calls.take_detail()))
        t.add(key + ["shortcut"], rle(seq))
    data = t.data()
    data["launches"], data["switches"] = launches, switches
    return data


def surface(K, monkeypatch):
    L = K._lib.load()
    return {"predicates": predicates(L), "errors": errors(L), "routes": routes(K, monkeypatch)}
