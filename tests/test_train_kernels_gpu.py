"""The training-step kernels (loss_ssim / loss_grad / loss_reduce, adam_step, densify_stats) and the seven kNN kernels on the
device, per element, against the restatements of tests/train_reference.py on the inputs of tests/train_cases.py.

Image loss.  The oracle is float64 autograd (loss_f64 / masked_loss_f64) on the float32 inputs the device holds.  The bound of
a case is measured reference against reference, never from the kernel: 4 x the largest deviation of the float32
transcription (loss_f32: the kernels' documented operation order in NumPy) from float64 ON THAT CASE, per quantity (every
gradient element, the loss, the mean SSIM), with a floor of 2^-22 of the quantity's largest reference magnitude.  The factor
4 is the margin test_pose_error_gpu.py uses for a different, equally valid rounding order (the compiler may contract
a * b + c where the transcription rounds twice).  mean |x - y'| and mean |alpha - m| are double sums of float32 differences
and are held to 2^-22 of their value; grad_alpha is lambda_a / (H W) in float times a sign and is compared bit for bit.

What float32 costs, per content family: the largest deviation over the family's cases (``python
tests/test_train_kernels_gpu.py`` prints this table on the CPU; test_train_kernels_host.py fails when it goes stale).  grad is
relative to the largest gradient element of the case, loss and SSIM are absolute; "2-D" is torch's float32 conv2d form of the
same loss (what the upstream loop computes), for the reader only:

    family             grad f32   (2-D)       loss f32   (2-D)       SSIM f32   (2-D)
    noise              5.72e-07   1.97e-06    1.29e-08   1.17e-07    5.18e-08   1.30e-07
    texture_impulses   1.33e-06   3.50e-06    3.40e-08   2.59e-07    8.88e-08   2.59e-07
    flat_object        3.98e-05   1.53e-04    1.58e-06   6.29e-06    1.58e-06   8.14e-06
    constant           7.31e-04   1.16e-03    6.64e-06   7.22e-06    3.32e-05   3.61e-05
    near_target        2.74e-04   8.82e-04    1.65e-06   3.57e-06    4.23e-06   5.25e-06
    out_of_range       3.36e-07   1.01e-06    3.83e-08   1.12e-07    1.28e-08   1.28e-08
    partly_equal       5.82e-07   1.53e-06    7.24e-09   6.40e-08    4.96e-08   6.40e-08
    masked_binary      4.55e-05   4.38e-05    1.44e-07   2.55e-07    7.29e-07   1.27e-06
    masked_soft        4.77e-07   1.59e-06    2.72e-08   9.20e-08    4.88e-08   1.49e-07

On flat images (a constant background, a render that has converged to it) the variance E[x^2] - mu^2 cancels to about 1e-7
against C2 = 9e-4: any float32 formulation is then only good to about 1e-4 of the SSIM term and 1e-3 of the largest gradient
element, and the bound of those cases says so.  Identical images are exact in every family: loss 0, gradient 0.

Adam: torch.optim.Adam(foreach=False) on the device, at most 1 ulp per step and no mismatch over the run.  Densification
statistics: bit-equal counts and radii, the norm within 2 ulp of float64, untouched rows bit-identical.  kNN: rtol 2e-5 against
knn_f64 (derivation at test_knn_matches_float64).
"""
import sys
from pathlib import Path

import numpy as np
import pytest

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
if __name__ == "__main__":
    sys.path.insert(0, str(HERE.parent))

import train_cases as TC                 # noqa: E402
import train_reference as TR             # noqa: E402

F32 = np.float32
GUARD = 4096
FLOOR = 2.0 ** -22
MARGIN = 4.0
QUANTITIES = ("grad", "loss", "ssim")
# largest |loss_f32 - loss_f64| per content family: grad relative to the case's largest gradient element, loss and ssim
# absolute (the "f32" columns of the table above)
MEASURED = {
    "noise": dict(grad=5.72e-07, loss=1.29e-08, ssim=5.18e-08),
    "texture_impulses": dict(grad=1.33e-06, loss=3.40e-08, ssim=8.88e-08),
    "flat_object": dict(grad=3.98e-05, loss=1.58e-06, ssim=1.58e-06),
    "constant": dict(grad=7.31e-04, loss=6.64e-06, ssim=3.32e-05),
    "near_target": dict(grad=2.74e-04, loss=1.65e-06, ssim=4.23e-06),
    "out_of_range": dict(grad=3.36e-07, loss=3.83e-08, ssim=1.28e-08),
    "partly_equal": dict(grad=5.82e-07, loss=7.24e-09, ssim=4.96e-08),
    "masked_binary": dict(grad=4.55e-05, loss=1.44e-07, ssim=7.29e-07),
    "masked_soft": dict(grad=4.77e-07, loss=2.72e-08, ssim=4.88e-08),
}

LOSS_CASES = {c["name"]: c for c in TC.loss_cases()}
MASKED_CASES = {c["name"]: c for c in TC.masked_cases()}


# ---- references and bounds (CPU) --------------------------------------------------------------------------------------------
def case_inputs(case):
    """dict(x, y, mask, alpha, bg, lam_a) of a loss case or a masked case (mask None: the unmasked loss)."""
    if "family" in case:
        x, y = TC.image_pair(case["family"], case["H"], case["W"], case["variant"])
        return dict(x=x, y=y, mask=None, alpha=None, bg=None, lam_a=0.0)
    d = TC.masked_inputs(case["kind"], case["H"], case["W"], case["bg"])
    if not case["use_alpha"]:
        d["alpha"] = None
    d["lam_a"] = case["lam_a"]
    return d


def _f64(inp, lam, restate=TR.masked_loss_f64):
    import torch
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a))
    loss, l1, ssim, al1, gx, ga = restate(t(inp["x"]), t(inp["alpha"]), t(inp["y"]), t(inp["mask"]), t(inp["bg"]), lam,
                                          inp["lam_a"])
    return dict(loss=loss, l1=l1, ssim=ssim, al1=al1, grad=gx.double().numpy(),
                grad_alpha=None if ga is None else ga.double().numpy().reshape(inp["x"].shape[1:]))


def deviations(f64, other):
    """Largest |other - f64| per asserted quantity; ``other``: loss_f32's dict or another _f64-style dict."""
    if "out" in other:
        o_loss, o_ssim = float(other["out"][0]), float(other["out"][2])
    else:
        o_loss, o_ssim = other["loss"], other["ssim"]
    return dict(grad=float(np.abs(other["grad"].astype(np.float64) - f64["grad"]).max()), loss=abs(o_loss - f64["loss"]),
                ssim=abs(o_ssim - f64["ssim"]))


_cache = {}


def reference(case, lam):
    """(inputs, float64 reference, float32 transcription, bounds) of a case at one lambda; computed once per process."""
    key = (case["name"], lam)
    if key not in _cache:
        inp = case_inputs(case)
        f64 = _f64(inp, lam)
        f32 = TR.masked_loss_f32(inp["x"], inp["alpha"], inp["y"], inp["mask"], inp["bg"], lam, inp["lam_a"])
        dev = deviations(f64, f32)
        scale = dict(grad=float(np.abs(f64["grad"]).max()), loss=abs(f64["loss"]), ssim=abs(f64["ssim"]))
        bound = {q: max(MARGIN * dev[q], FLOOR * scale[q]) for q in QUANTITIES}
        bound["l1"] = FLOOR * f64["l1"]
        bound["al1"] = FLOOR * f64["al1"]
        _cache[key] = (inp, f64, f32, bound)
    return _cache[key]


def case_family(case):
    return case["family"] if "family" in case else "masked_" + case["kind"]


def case_lambdas(case):
    return case["lams"] if "family" in case else (case["lam"],)


def measure(with_torch_f32=False, verbose=False):
    """{family: {grad, loss, ssim}}: the largest deviation of loss_f32 from loss_f64 over the family's cases and lambdas
    (grad relative to the case's largest gradient element); with_torch_f32 adds torch's float32 2-D form as "<q>_2d"."""
    worst = {}
    for case in list(LOSS_CASES.values()) + list(MASKED_CASES.values()):
        w = worst.setdefault(case_family(case), {})
        for lam in case_lambdas(case):
            inp, f64, f32, _ = reference(case, lam)
            devs = {"": deviations(f64, f32)}
            if with_torch_f32:
                devs["_2d"] = deviations(f64, _f64(inp, lam, TR.loss_torch_f32))
            gmax = float(np.abs(f64["grad"]).max())
            for suffix, d in devs.items():
                d = dict(d, grad=d["grad"] / gmax if gmax > 0 else d["grad"])
                for q in QUANTITIES:
                    w[q + suffix] = max(w.get(q + suffix, 0.0), d[q])
                if verbose:
                    print(f"    {case['name']:34s} lam {lam:3.1f} {suffix or '_f32':4s} " +
                          " ".join(f"{q} {d[q]:.3e}" for q in QUANTITIES))
    return worst


# ---- raw calls inside guard bands ---------------------------------------------------------------------------------------
def _guarded(n, dtype, fill):
    import torch
    full = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
    return full, full[GUARD:GUARD + n]


def _intact(full, n, fill, what):
    assert bool((full[:GUARD] == fill).all()) and bool((full[GUARD + n:] == fill).all()), f"{what} guard overwritten"


def run_loss(inp, lam, want_grad=True, want_grad_alpha=True):
    """pgr_image_loss (mask None) or pgr_image_loss_masked through the C ABI: the workspace exactly
    pgr_*_workspace_bytes long and every output inside guard bands, which must be intact afterwards.  Returns dict(out [3] or
    [4], grad or None, grad_alpha or None) as NumPy arrays."""
    import torch
    from pegasus_amd import _lib
    L = _lib.lib()
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, F32)).cuda()
    x, y, m, a, bg = (up(inp[k]) for k in ("x", "y", "mask", "alpha", "bg"))
    _, H, W = inp["x"].shape
    masked = m is not None
    nbytes = int((L.pgr_image_loss_masked_workspace_bytes if masked else L.pgr_image_loss_workspace_bytes)(H, W))
    assert nbytes > 0
    n_out, n = (4 if masked else 3), 3 * H * W
    out_f, out = _guarded(n_out, torch.float32, 12345.0)
    grad_f, grad = _guarded(n, torch.float32, 12345.0)
    ga_f, ga = _guarded(H * W, torch.float32, 12345.0)
    ws_f, ws = _guarded(nbytes, torch.uint8, 0xA5)
    want_grad_alpha = want_grad_alpha and a is not None
    p = _lib.ptr
    stream = _lib.stream_ptr(x.device)
    if masked:
        rc = L.pgr_image_loss_masked(p(x), p(y), p(m), p(bg), p(a), H, W, float(lam), float(inp["lam_a"]), p(out),
                                     p(grad) if want_grad else None, p(ga) if want_grad_alpha else None, p(ws), nbytes, stream)
    else:
        rc = L.pgr_image_loss(p(x), p(y), H, W, float(lam), p(out), p(grad) if want_grad else None, p(ws), nbytes, stream)
    _lib.check(rc, "pgr_image_loss")
    torch.cuda.synchronize()
    _intact(out_f, n_out, 12345.0, "out")
    _intact(grad_f, n, 12345.0, "grad")
    _intact(ga_f, H * W, 12345.0, "grad_alpha")
    _intact(ws_f, nbytes, 0xA5, "workspace")
    if not want_grad:
        assert bool((grad == 12345.0).all()), "grad written without being asked for"
    if not want_grad_alpha:
        assert bool((ga == 12345.0).all()), "grad_alpha written without being asked for"
    return dict(out=out.cpu().numpy(), grad=grad.reshape(3, H, W).cpu().numpy() if want_grad else None,
                grad_alpha=ga.reshape(H, W).cpu().numpy() if want_grad_alpha else None)


def run_loss_twice(inp, lam, **kw):
    got, again = run_loss(inp, lam, **kw), run_loss(inp, lam, **kw)
    for k, v in got.items():
        assert (v is None) == (again[k] is None) and (v is None or v.tobytes() == again[k].tobytes()), f"two runs differ: {k}"
    return got


def check_loss(case, lam, got):
    inp, f64, _, bound = reference(case, lam)
    fam, name = case_family(case), case["name"]
    pairs = [("loss", float(got["out"][0]), f64["loss"]), ("l1", float(got["out"][1]), f64["l1"]),
             ("ssim", float(got["out"][2]), f64["ssim"])]
    if len(got["out"]) == 4:
        pairs.append(("al1", float(got["out"][3]), f64["al1"]))
    failures = []
    for q, g, want in pairs:
        dev = abs(g - want)
        print(f"RATIO {fam:16s} {name:34s} lam {lam:3.1f} {q:5s} dev {dev:.3e} bound {bound[q]:.3e} "
              f"ratio {dev / bound[q] if bound[q] > 0 else float(dev > 0):.3f}")
        if not dev <= bound[q]:
            failures.append((q, g, want, dev, bound[q]))
    if got["grad"] is not None:
        assert got["grad"].dtype == F32 and np.isfinite(got["grad"]).all()
        dev = np.abs(got["grad"].astype(np.float64) - f64["grad"])
        worst = np.unravel_index(int(np.argmax(dev)), dev.shape)
        print(f"RATIO {fam:16s} {name:34s} lam {lam:3.1f} grad  dev {dev.max():.3e} bound {bound['grad']:.3e} "
              f"ratio {dev.max() / bound['grad'] if bound['grad'] > 0 else float(dev.max() > 0):.3f}")
        if not (dev <= bound["grad"]).all():                                   # every element, one bound per case
            failures.append(("grad", worst, float(got["grad"][worst]), float(f64["grad"][worst]), float(dev.max()), bound["grad"]))
    assert not failures, (name, lam, failures)
    if got["grad_alpha"] is not None:
        _, H, W = inp["x"].shape
        d = inp["alpha"].astype(np.float64) - inp["mask"].astype(np.float64)
        want = F32(inp["lam_a"] / (float(H) * float(W))) * np.sign(d).astype(F32)
        assert got["grad_alpha"].view(np.uint32).tolist() == want.view(np.uint32).tolist(), (name, "grad_alpha bits")
        if inp["lam_a"] > 0:
            assert np.allclose(got["grad_alpha"], f64["grad_alpha"], rtol=1e-6, atol=0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(LOSS_CASES))
def test_image_loss_per_element(gpu_device, name):
    case = LOSS_CASES[name]
    for lam in case["lams"]:
        inp = reference(case, lam)[0]
        check_loss(case, lam, run_loss_twice(inp, lam))
    out_only = run_loss(inp, case["lams"][-1], want_grad=False)               # without a gradient: the same value
    assert out_only["out"].tobytes() == run_loss(inp, case["lams"][-1])["out"].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(MASKED_CASES))
def test_masked_loss_per_element(gpu_device, name):
    case = MASKED_CASES[name]
    inp = reference(case, case["lam"])[0]
    got = run_loss_twice(inp, case["lam"], want_grad=case["want_grad"], want_grad_alpha=case["want_grad_alpha"])
    check_loss(case, case["lam"], got)


@pytest.mark.gpu
@pytest.mark.parametrize("hw", TC.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_loss_of_identical_images_is_exactly_zero(gpu_device, hw):
    """x == y (and x == y', alpha == mask): loss 0, SSIM term 1 within 2^-22, every gradient element 0 -- in the content
    families of the trainer too, not only on noise."""
    H, W = hw
    for fam in ("noise", "flat_object", "out_of_range"):
        x, _ = TC.image_pair(fam, H, W)
        for lam in (0.0, 0.2, 1.0):
            got = run_loss(dict(x=x, y=x.copy(), mask=None, alpha=None, bg=None, lam_a=0.0), lam)
            assert got["out"][0] == 0.0 and got["out"][1] == 0.0 and abs(float(got["out"][2]) - 1.0) <= FLOOR, (fam, lam, got["out"])
            assert not got["grad"].any(), (fam, lam, float(np.abs(got["grad"]).max()))
    for bg in TC.BACKGROUNDS:
        d = TC.masked_inputs("binary", H, W, bg)
        yt = TR.masked_target_f32(d["y"], d["mask"], d["bg"])
        assert np.array_equal(yt, np.where(d["mask"][None] > 0, d["y"], d["bg"][:, None, None]))   # exact for a 0/1 mask
        got = run_loss(dict(d, x=yt, alpha=d["mask"].copy(), lam_a=0.5), 0.2)
        assert got["out"][0] == 0.0 and got["out"][1] == 0.0 and got["out"][3] == 0.0, (bg, got["out"])
        assert abs(float(got["out"][2]) - 1.0) <= FLOOR and not got["grad"].any() and not got["grad_alpha"].any()


@pytest.mark.gpu
@pytest.mark.parametrize("hw", TC.FAMILY_SHAPES["partly_equal"], ids=lambda s: f"{s[0]}x{s[1]}")
def test_l1_gradient_is_exact(gpu_device, hw):
    """lambda = 0: the gradient is sign(x - y) times float((1 - 0) / n), bit for bit; exactly 0 on the equal half."""
    H, W = hw
    x, y = TC.image_pair("partly_equal", H, W)
    got = run_loss(dict(x=x, y=y, mask=None, alpha=None, bg=None, lam_a=0.0), 0.0)
    assert W // 2 > 0 and not got["grad"][:, :, : W // 2].any()
    want = F32(1.0 / (3.0 * H * W)) * np.sign(x.astype(np.float64) - y.astype(np.float64)).astype(F32)
    assert np.array_equal(got["grad"], want)
    assert (got["grad"][:, :, W // 2:] != 0).all()


@pytest.mark.gpu
def test_gradient_scales_with_grad_output(gpu_device):
    import torch
    from pegasus_amd.train_ops import ImageLoss, MaskedImageLoss
    x, y = (torch.from_numpy(t).to(gpu_device) for t in TC.image_pair("texture_impulses", 21, 27))
    a = x.clone().requires_grad_(True)
    ImageLoss.apply(a, y, 0.2).backward()
    b = x.clone().requires_grad_(True)
    (3.0 * ImageLoss.apply(b, y, 0.2)).backward()
    torch.testing.assert_close(b.grad, 3.0 * a.grad, rtol=1e-6, atol=0)
    d = {k: torch.from_numpy(v).to(gpu_device) for k, v in TC.masked_inputs("binary", 21, 27, TC.BACKGROUNDS[1]).items()}
    grads = []
    for scale in (1.0, 3.0):
        xs, al = d["x"].clone().requires_grad_(True), d["alpha"].clone().requires_grad_(True)
        (scale * MaskedImageLoss.apply(xs, al, d["y"], d["mask"], d["bg"], 0.2, 0.5)).backward()
        grads.append((xs.grad, al.grad))
    torch.testing.assert_close(grads[1][0], 3.0 * grads[0][0], rtol=1e-6, atol=0)
    torch.testing.assert_close(grads[1][1], 3.0 * grads[0][1], rtol=1e-6, atol=0)


# ---- Adam -------------------------------------------------------------------------------------------------------------------
ADAM_LAUNCHES = {"sixteen": 1, "sixteen_empties": 2, "seventeen": 2, "thirty_three": 3}


def _t_ulps(a, b):
    import torch
    ia, ib = a.contiguous().view(torch.int32).long(), b.contiguous().view(torch.int32).long()
    ia = torch.where(ia < 0, -(ia & 0x7fffffff), ia)
    ib = torch.where(ib < 0, -(ib & 0x7fffffff), ib)
    return (ia - ib).abs()


@pytest.mark.gpu
@pytest.mark.parametrize("start", TC.ADAM_START_STEPS)
@pytest.mark.parametrize("layout", list(ADAM_LAUNCHES))
def test_fused_adam_tables_edges_and_late_steps(gpu_device, monkeypatch, layout, start):
    """FusedAdam against torch.optim.Adam(foreach=False) on the device, as test_fused_adam_matches_torch_adam: at most 1 ulp
    per step, no mismatch over the run, equal ``step``, version counters bumped -- with parameters at the 1024-element
    workgroup boundary, a full 16-entry table, a second and a third launch, empty parameters, a group of three, a parameter
    without a gradient, two pairs of betas / eps, states preset at step 1, 2, 1000 and 29999, and gradients that are all zero
    (from the start: the parameter keeps its bits; after a history), 1e-12 .. 1e6 with both signs."""
    import torch
    from pegasus_amd import _lib
    from pegasus_amd.train_ops import FusedAdam
    groups = TC.adam_layouts()[layout]
    rng = np.random.default_rng(1000 * start + len(groups))
    dev = lambda a: torch.from_numpy(a).to(gpu_device)
    ours, ref, kinds, g_ours, g_ref = [], [], [], [], []
    for g in groups:
        init = [rng.standard_normal(n).astype(F32) for n in g["sizes"]]
        po = [torch.nn.Parameter(dev(t.copy())) for t in init]
        pr = [torch.nn.Parameter(dev(t.copy())) for t in init]
        ours += po; ref += pr; kinds += g["kinds"]
        g_ours.append({"params": po, "lr": g["lr"], "betas": g["betas"], "eps": g["eps"]})
        g_ref.append({"params": pr, "lr": g["lr"], "betas": g["betas"], "eps": g["eps"]})
    opt = FusedAdam(g_ours, lr=0.0, eps=1e-15)
    topt = torch.optim.Adam(g_ref, lr=0.0, eps=1e-15, foreach=False)
    if start:
        for p, q, kind in zip(ours, ref, kinds):
            m, v = TC.adam_history(kind, p.numel(), start, rng)
            for o, t in ((opt, p), (topt, q)):
                o.state[t] = {"step": torch.tensor(float(start)), "exp_avg": dev(m.copy()), "exp_avg_sq": dev(v.copy())}
    L = _lib.lib()
    real, calls = L.pgr_adam_step, []
    monkeypatch.setattr(L, "pgr_adam_step", lambda table, n, *rest: (calls.append(n), real(table, n, *rest))[1], raising=False)
    frozen = [(p.detach().clone(), {k: v.clone() for k, v in opt.state[p].items()}) for p in ours]
    mismatched = elements = 0
    for k in range(TC.ADAM_STEPS):
        for p, q, kind in zip(ours, ref, kinds):
            g = TC.adam_gradient(kind, p.numel(), k, rng)
            p.grad, q.grad = (None, None) if g is None else (dev(g.copy()), dev(g.copy()))
        versions = [p._version for p in ours]
        del calls[:]
        opt.step()
        topt.step()
        assert len(calls) == ADAM_LAUNCHES[layout] and max(calls) <= _lib.PGR_ADAM_MAX_GROUPS, calls
        if layout == "sixteen":
            assert calls == [16]
        for i, (p, q, kind) in enumerate(zip(ours, ref, kinds)):
            so, st = opt.state[p], topt.state[q]
            if kind == "none":                                               # no gradient: nothing moves, as in torch
                assert p._version == versions[i] and torch.equal(p, frozen[i][0]) and torch.equal(q, p)
                assert set(so) == set(st) == set(frozen[i][1])
                assert all(torch.equal(so[key], frozen[i][1][key]) and torch.equal(st[key].cpu(), so[key].cpu()) for key in so)
                continue
            assert p._version > versions[i]
            assert float(so["step"]) == float(st["step"]) == start + k + 1
            for a, b in ((p.data, q.data), (so["exp_avg"], st["exp_avg"]), (so["exp_avg_sq"], st["exp_avg_sq"])):
                if a.numel():
                    assert bool(torch.isfinite(a).all())
                    u = _t_ulps(a, b)
                    assert int(u.max()) <= 1, (layout, start, k, i, kind, int(u.max()))
                    mismatched += int((u > 0).sum())
                    elements += a.numel()
                    b.copy_(a)
            if kind == "zero":                                               # g = 0 on zero moments: 0 / eps, not NaN
                assert torch.equal(p.data, frozen[i][0]) and not so["exp_avg"].any() and not so["exp_avg_sq"].any()
    print(f"\nFusedAdam {layout} from step {start + 1}: {mismatched} of {elements} values off by 1 ulp")
    assert mismatched == 0


# ---- densification statistics ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", TC.DENSIFY_N)
def test_densify_stats_per_row(gpu_device, n):
    import torch
    from pegasus_amd.train_ops import densify_stats
    for columns in TC.DENSIFY_COLUMNS:
        for variant in ((0, 1) if n == 1 else (0,)):
            d = TC.densify_inputs(n, columns, variant)
            t = {k: torch.from_numpy(v.copy()).to(gpu_device) for k, v in d.items()}
            vis = t["radii"] > 0
            e_denom, e_max = t["denom"].clone(), t["max_r"].clone()
            e_denom[vis] += 1
            e_max[vis] = torch.max(e_max[vis], t["radii"][vis].float())
            densify_stats(t["vgrad"], t["radii"], t["accum"], t["denom"], t["max_r"])
            got = {k: t[k].cpu().numpy() for k in ("accum", "denom", "max_r")}
            bits = lambda a: np.ascontiguousarray(a).view(np.int32).reshape(-1)
            assert np.array_equal(bits(got["denom"]), bits(e_denom.cpu().numpy())), (n, columns)
            assert np.array_equal(bits(got["max_r"]), bits(e_max.cpu().numpy())), (n, columns)
            hidden = d["radii"] <= 0
            for k in ("accum", "denom", "max_r"):                               # untouched rows keep their bits, payloads too
                assert np.array_equal(bits(got[k])[hidden], bits(d[k])[hidden]), (n, columns, k)
            want, _, _ = TR.densify_f64(d["vgrad"], d["radii"], d["accum"], d["denom"], d["max_r"])
            shown = ~hidden
            assert np.isfinite(got["accum"].reshape(-1)[shown]).all()
            u = TR.ulps(got["accum"].reshape(-1)[shown], want[shown].astype(F32))
            assert u.size == 0 or int(u.max()) <= 2, (n, columns, int(u.max()))
            if n > 1:
                assert shown.any() and hidden.any() and (d["radii"] == 2 ** 24 + 1).any()
                assert got["max_r"][0] == 2.0 ** 24


# ---- kNN --------------------------------------------------------------------------------------------------------------------
def run_knn(pts):
    """pgr_knn_mean_dist2 through the C ABI, the output and the exactly sized workspace inside guard bands."""
    import torch
    from pegasus_amd import _lib
    L = _lib.lib()
    n = len(pts)
    xyz = torch.from_numpy(np.ascontiguousarray(pts, F32)).cuda()
    nbytes = int(L.pgr_knn_workspace_bytes(n))
    out_f, out = _guarded(n, torch.float32, 12345.0)
    ws_f, ws = _guarded(nbytes, torch.uint8, 0xA5)
    _lib.check(L.pgr_knn_mean_dist2(n, _lib.ptr(xyz), _lib.ptr(out), _lib.ptr(ws), nbytes, _lib.stream_ptr(xyz.device)),
               "pgr_knn_mean_dist2")
    torch.cuda.synchronize()
    _intact(out_f, n, 12345.0, "out")
    _intact(ws_f, nbytes, 0xA5, "workspace")
    return out.cpu().numpy()


def knn_facade(pts, device):
    import torch
    from pegasus_amd.knn import distCUDA2
    return distCUDA2(torch.from_numpy(pts).to(device)).cpu().numpy()


KNN_RTOL, KNN_ATOL = 2e-5, 1e-12


@pytest.mark.gpu
@pytest.mark.parametrize("name", TC.KNN_CASES)
def test_knn_matches_float64(gpu_device, name):
    """rtol 2e-5 against knn_f64 on the same float32 points.  Each squared distance is three float32 differences (one
    rounding each, 2^-24 relative), three squares and two sums: a few 2^-24 = 6e-8 each.  The shell search stops once the third
    best distance is within 0.99999 r cells; the cell index of a point is itself rounded (float32 subtract and multiply), so a
    point that index arithmetic puts r + 1 cells away can be nearer than r cells by a few 1e-6 of a cell: the search may then
    keep a third neighbour whose squared distance exceeds the true one by at most 1 - 0.99999^2 = 2e-5 of itself, which is
    at most 7e-6 of the mean of the three."""
    pts = TC.knn_points(name)
    n = len(pts)
    raw = n <= 5000                                   # guard bands at the small and ragged sizes, the facade beyond
    got = run_knn(pts) if raw else knn_facade(pts, gpu_device)
    if raw:
        assert got.tobytes() == run_knn(pts).tobytes(), "two runs differ"
        assert got.tobytes() == knn_facade(pts, gpu_device).tobytes()
    assert got.shape == (n,) and got.dtype == F32
    if n < 4:
        assert (got > 1e30).all()                      # fewer than 3 neighbours: FLT_MAX terms, as upstream
        return
    assert np.isfinite(got).all()
    ref = TR.knn_f64(pts, brute=name in ("identical", "two_groups") or n <= 5)
    np.testing.assert_allclose(got, ref, rtol=KNN_RTOL, atol=KNN_ATOL)
    if name.startswith("lattice"):                     # every third neighbour at exactly one cell: h^2
        k = int(name[7])
        assert TC.knn_grid_target(n) == k - 1          # cell size h: every point on a cell boundary
        assert (TR.ulps(got, np.full(n, TC.LATTICE_H ** 2, F32)) <= 1).all() and np.allclose(ref, TC.LATTICE_H ** 2, rtol=1e-12)
    if name in ("identical", "two_groups"):
        assert not got.any() and not ref.any()
    if name == "uniform5000":
        assert TC.knn_grid_target(n) == 14             # 2744 cells: two full scan chunks and a ragged one
    if name == "uniform150000":
        assert TC.knn_grid_target(n) == 43


@pytest.mark.gpu
def test_knn_at_128_cells_per_axis(gpu_device):
    """4 096 767 points (the smallest n with KNN_MAX_GRID = 128 cells per axis: a 2 M-cell single-workgroup scan, cell
    indices up to 127) in a box from -8.3 over 18.6 per axis.  Checked: 2000 sampled points and up to 2000 points within 1e-4
    of the extent from a face of the bounding box (the clamp of the upper faces), against scipy's k-d tree over ALL points in
    float64 (built unbalanced and uncompacted: about 2 s on the host)."""
    pts = TC.knn_points("big")
    assert TC.knn_grid_target(len(pts)) == 128 and TC.knn_grid_target(len(pts) - 1) == 127
    got = knn_facade(pts, gpu_device)
    sampled, near = TC.knn_big_queries(pts)
    assert len(sampled) == 2000 and 500 <= len(near) <= 2000
    q = np.concatenate([sampled, near])
    ref = TR.knn_f64(pts, queries=q)
    dev = np.abs(got[q] - ref) / ref
    print(f"\nkNN at 128 cells: largest relative deviation {dev.max():.3e} over {len(q)} points (bound {KNN_RTOL:.0e})")
    np.testing.assert_allclose(got[q], ref, rtol=KNN_RTOL, atol=KNN_ATOL)
    assert np.isfinite(got).all() and (got > 0).all()


def print_table():
    worst = measure(with_torch_f32=True)
    print(f"    {'family':18s} grad f32   (2-D)       loss f32   (2-D)       SSIM f32   (2-D)")
    for fam, w in worst.items():
        print(f"    {fam:18s} " + "    ".join(f"{w[q]:.2e}   {w[q + '_2d']:.2e}" for q in QUANTITIES))
    print("MEASURED = {")
    for fam, w in worst.items():
        print(f'    "{fam}": dict(' + ", ".join(f"{q}={w[q]:.2e}" for q in QUANTITIES) + "),")
    print("}")


if __name__ == "__main__":
    print_table()
