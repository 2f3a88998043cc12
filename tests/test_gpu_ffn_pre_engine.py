"""ZV_FFN=3 through the engine: the conv + SelfAttention out-projection as the first phase of the
fused FeedForward behind it (zv_ffn.inc PRE; zv_engine layer<1>), at test_gpu_ffn.py's shapes.

ZV_FFN=3 differs from ZV_FFN=2 in where the out-projection's sum meets the residual (initial
accumulators instead of a GEMM epilogue) and in x being rounded from registers: roundings of the
same kind as between the other arms, so each arm is held to its mode's bar against the fp32 oracle
and the two arms to twice the bar against each other (test_gpu_ffn.py's rule for arms with
independent roundings).  The profiler report shows which launches ran."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

BAR = {"bf16": 5e-2, "fp16": 1e-3}


def _velocity(monkeypatch, env, precision, B=2, T=203, lens=(203, 150), t=0.4, seed=11, report=False):
    from zipvoice_amd import engine
    from zipvoice_amd.config import default_config
    from zipvoice_amd.models import build_model
    from zipvoice_amd.weights import synthetic_state_dict
    cfg = default_config("zipvoice")
    sd = synthetic_state_dict(cfg, 0)
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, T, cfg.feat_dim), dtype=np.float32)
    tc = rng.standard_normal(x.shape, dtype=np.float32)
    sc = rng.standard_normal(x.shape, dtype=np.float32)
    pm = np.arange(T)[None] >= np.array(lens)[:, None]
    for k in ("ZV_FFN", "ZV_FFN_MIN_ROWS", "ZV_SPLIT_STREAMS", "ZV_FFN_PERSIST", "ZV_GRAPH"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m = build_model(cfg, precision=precision)
    m.load_state_dict(sd)
    m = m.to("cuda:0")
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    args = (t, 1.0, cu(x), cu(tc), cu(sc), cu(pm))
    rep = None
    if report:
        engine.profile(True)
    try:
        out = m.engine.velocity(*args).cpu().numpy()
        if report:
            rep = engine.profile_report()
    finally:
        if report:
            engine.profile(False)
    del m
    return out, rep, (cfg, sd, x, tc, sc, pm, t)


def _launches(rep, tag):
    return sum(v["launches"] for k, v in rep.items() if k == tag or k.startswith(tag + "["))


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_pre_projection_vs_oracle_and_ffn2(monkeypatch, precision):
    from oracle.zipvoice_np import ZipVoiceOracle
    outs, reps = {}, {}
    for ffn in ("2", "3"):
        outs[ffn], reps[ffn], inp = _velocity(monkeypatch, {"ZV_FFN": ffn, "ZV_FFN_MIN_ROWS": "0"}, precision,
                                              report=True)
    cfg, sd, x, tc, sc, pm, t = inp
    ref = ZipVoiceOracle(cfg, sd).velocity(np.float32(t), x, tc, sc, pm, 1.0)
    valid = ~pm
    bar = BAR[precision]
    for ffn, o in outs.items():
        e = np.abs(o - ref)[valid]
        print(f"{precision} ZV_FFN={ffn}: vs oracle mean {e.mean():.3e} max {e.max():.3e}; "
              f"resid_rv launches {_launches(reps[ffn], 'gemm_bf16_resid_rv')}, "
              f"ffn {_launches(reps[ffn], 'ffn_bf16')}, ffn_norm {_launches(reps[ffn], 'ffn_norm_bf16')}")
        assert np.isfinite(o).all()
        assert e.mean() < bar
    d = np.abs(outs["3"] - outs["2"])[valid].mean()
    print(f"{precision} ZV_FFN=3 vs 2: mean {d:.3e}")
    assert d < 2 * bar
    # the K-concatenated out-projection ran as its own launch with ZV_FFN=2, not at all with 3; the
    # fused FeedForward launches are the same ones
    assert _launches(reps["2"], "gemm_bf16_resid_rv") > 0
    assert _launches(reps["3"], "gemm_bf16_resid_rv") == 0
    for tag in ("ffn_bf16", "ffn_norm_bf16"):
        assert _launches(reps["3"], tag) == _launches(reps["2"], tag) > 0, tag


def test_pre_projection_split_streams_bitwise(monkeypatch):
    """Default settings (ZV_FFN=3, the persistent line schedule, the default row thresholds) at
    test_gpu_split_streams.py's persistent-schedule shape: one row block per block on one stream,
    lines on one stream, lines on the split decoder's three streams.  Lines cut row blocks, whose P
    items hand x over through the stream's 16-bit copy: bitwise equal velocities."""
    B, T = 16, 1219
    lens = tuple(1219 - 37 * i for i in range(B))
    outs = []
    for env in ({"ZV_SPLIT_STREAMS": "1", "ZV_FFN_PERSIST": "0"}, {"ZV_SPLIT_STREAMS": "1"}, {"ZV_SPLIT_STREAMS": "3"}):
        o, rep, _ = _velocity(monkeypatch, env, "bf16", B=B, T=T, lens=lens, t=0.3, seed=5, report=len(outs) == 1)
        if rep is not None:   # (stacks under the row threshold keep the unfused pair and its linears)
            assert _launches(rep, "ffn_norm_bf16") > 0
        outs.append(o)
    for j, o in enumerate(outs[1:], 1):
        assert np.isfinite(o).all()
        assert np.array_equal(o, outs[0]), (j, np.abs(o - outs[0]).max())
