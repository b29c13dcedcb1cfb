"""The decision unet.py makes per adapted projection, tabled: proj_form over every site x adapter state, and the
boundary of each clause of fp8_site_ok.  The expectations are literal (DESIGN "Adapted projections"), not a second
copy of the rule."""
import itertools

import pytest

from pairwise_sample_optimization_amd import unet as U

# (lora_on, dora, merged, ok8, "tail" in FP8_KINDS) -> form, every state written out, per class of site.
# qkv, q2: the sites with the "fp8 base, bf16 LoRA term" diagnostic form
DIAG = {
    (True, False, False, True, False): "fp8_base_bf16_tail", (True, False, True, True, False): "fp8_base_bf16_tail",
    (True, True, False, True, False): "fp8_base_bf16_tail", (True, True, True, True, False): "fp8_base_bf16_tail",
    (True, False, False, True, True): "fp8_tail", (True, False, True, True, True): "fp8_tail",
    (True, True, False, True, True): "fp8_tail", (True, True, True, True, True): "fp8_tail",
    (True, True, False, False, False): "dora", (True, True, True, False, False): "dora",
    (True, True, False, False, True): "dora", (True, True, True, False, True): "dora",
    (True, False, False, False, False): "lora", (True, False, True, False, False): "lora",
    (True, False, False, False, True): "lora", (True, False, True, False, True): "lora",
    (False, False, False, True, False): "fp8", (False, False, True, True, False): "fp8",
    (False, True, False, True, False): "fp8", (False, True, True, True, False): "fp8",
    (False, False, False, True, True): "fp8", (False, False, True, True, True): "fp8",
    (False, True, False, True, True): "fp8", (False, True, True, True, True): "fp8",
    (False, False, True, False, False): "merged", (False, True, True, False, False): "merged",
    (False, False, True, False, True): "merged", (False, True, True, False, True): "merged",
    (False, False, False, False, False): "plain", (False, True, False, False, False): "plain",
    (False, False, False, False, True): "plain", (False, True, False, False, True): "plain",
}
# o1, o2: no diagnostic form -- the e4m3 tail whether or not "tail" is in FP8_KINDS
OUT = dict(DIAG)
OUT.update({(True, False, False, True, False): "fp8_tail", (True, False, True, True, False): "fp8_tail",
            (True, True, False, True, False): "fp8_tail", (True, True, True, True, False): "fp8_tail"})
# kv2: never an fp8 form -- ok8 changes nothing
KV = {
    (True, True, False, True, False): "dora", (True, True, True, True, False): "dora",
    (True, True, False, True, True): "dora", (True, True, True, True, True): "dora",
    (True, True, False, False, False): "dora", (True, True, True, False, False): "dora",
    (True, True, False, False, True): "dora", (True, True, True, False, True): "dora",
    (True, False, False, True, False): "lora", (True, False, True, True, False): "lora",
    (True, False, False, True, True): "lora", (True, False, True, True, True): "lora",
    (True, False, False, False, False): "lora", (True, False, True, False, False): "lora",
    (True, False, False, False, True): "lora", (True, False, True, False, True): "lora",
    (False, False, True, True, False): "merged", (False, True, True, True, False): "merged",
    (False, False, True, True, True): "merged", (False, True, True, True, True): "merged",
    (False, False, True, False, False): "merged", (False, True, True, False, False): "merged",
    (False, False, True, False, True): "merged", (False, True, True, False, True): "merged",
    (False, False, False, True, False): "plain", (False, True, False, True, False): "plain",
    (False, False, False, True, True): "plain", (False, True, False, True, True): "plain",
    (False, False, False, False, False): "plain", (False, True, False, False, False): "plain",
    (False, False, False, False, True): "plain", (False, True, False, False, True): "plain",
}
EXPECT = {"qkv": DIAG, "q2": DIAG, "o1": OUT, "o2": OUT, "kv2": KV}


def test_site_table():
    got = {k: (s.groups, s.fp8_kind, s.bf16_tail, s.gA, s.gB) for k, s in U.SITES.items()}
    assert got == {"qkv": (3, "qkv", True, "attn1.A_qkv", "attn1.B_qkv"),
                   "o1": (1, "out", False, "attn1.A_o", "attn1.B_o"),
                   "q2": (1, "q2", True, "attn2.A_q", "attn2.B_q"),
                   "kv2": (2, None, False, "attn2.A_kv", "attn2.B_kv"),
                   "o2": (1, "out", False, "attn2.A_o", "attn2.B_o")}
    s = U.SITES["kv2"]  # the per-block namespace fields keep LoraState's names
    assert (s.A, s.sB, s.At, s.sBt, s.g, s.n, s.dm) == ("A_kv2", "sB_kv2", "At_kv2", "sBt_kv2", "g_kv2", "n_kv2",
                                                         "dm_kv2")


@pytest.mark.parametrize("site", ["qkv", "o1", "q2", "kv2", "o2"])
def test_proj_form_table(site):
    table = EXPECT[site]
    states = list(itertools.product((False, True), repeat=5))
    assert sorted(table) == sorted(states), "the table covers every state exactly once"
    for lora_on, dora, merged, ok8, tail in states:
        got = U.proj_form(site, lora_on, dora, merged, ok8, tail)
        assert got == table[lora_on, dora, merged, ok8, tail], (site, lora_on, dora, merged, ok8, tail, got)


def test_fp8_site_ok_clauses(monkeypatch):
    monkeypatch.setattr(U, "FP8_KINDS", {"q2", "ff", "tail"})
    monkeypatch.setattr(U, "FP8_MIN_TILES", 0)
    ok = U.fp8_site_ok
    # (fp8_on, kind, n_out, k_in, lora_on, r_pad, M)
    assert ok(True, "q2", 256, 128, False, 0, 1) is True
    assert ok(False, "q2", 256, 128, False, 0, 1) is False       # fp8 forward off
    assert ok(True, "qkv", 256, 128, False, 0, 1) is False       # kind not selected
    assert ok(True, None, 256, 128, False, 0, 1) is False        # a site without an fp8 kind (kv2)
    assert ok(True, "q2", 255, 128, False, 0, 4096) is False     # n_out % 256
    assert ok(True, "q2", 512, 128, False, 0, 1) is True
    assert ok(True, "q2", 256, 64, False, 0, 1) is False         # k_in % 128
    assert ok(True, "q2", 256, 128, True, 8, 1) is False         # adapter on: the fp8 tail needs r_pad % 16 == 0
    assert ok(True, "q2", 256, 128, True, 16, 1) is True
    assert ok(True, "q2", 256, 128, False, 8, 1) is True         # adapter off: the rank does not matter
    assert ok(True, "q2", 256, 128, False, 16, 1) is True


def test_fp8_site_ok_occupancy_rule(monkeypatch):
    """ceil(M / 256) * (n_out // 256) >= FP8_MIN_TILES over the FULL row count, read at call time."""
    monkeypatch.setattr(U, "FP8_KINDS", {"q2"})
    monkeypatch.setattr(U, "FP8_MIN_TILES", 192)
    ok = lambda M, n_out: U.fp8_site_ok(True, "q2", n_out, 128, False, 0, M)
    assert ok(256 * 48, 1024) is True            # 48 x 4 = 192 tiles: at the bar
    assert ok(256 * 47 + 1, 1024) is True        # a started row tile counts: ceil -> 48 x 4
    assert ok(256 * 47, 1024) is False           # 47 x 4 = 188
    assert ok(256 * 191, 256) is False           # one below
    assert ok(256 * 192, 256) is True
    monkeypatch.setattr(U, "FP8_MIN_TILES", 0)   # no occupancy rule
    assert ok(1, 256) is True
    monkeypatch.setattr(U, "FP8_MIN_TILES", 2)
    assert ok(256, 256) is False and ok(257, 256) is True


def test_fp8_kinds_reassigned_without_reimport():
    """Tools assign unet.FP8_KINDS directly (tools/fp8_kinds.py): the next call sees it."""
    saved = U.FP8_KINDS
    try:
        U.FP8_MIN_TILES, tiles = 0, U.FP8_MIN_TILES
        U.FP8_KINDS = {"out"}
        assert U.fp8_site_ok(True, "out", 256, 128, False, 0, 1) is True
        assert U.fp8_site_ok(True, "q2", 256, 128, False, 0, 1) is False
        U.FP8_KINDS = {"q2"}
        assert U.fp8_site_ok(True, "out", 256, 128, False, 0, 1) is False
        assert U.fp8_site_ok(True, "q2", 256, 128, False, 0, 1) is True
    finally:
        U.FP8_KINDS, U.FP8_MIN_TILES = saved, tiles


def test_fp8_geglu_pays_reads_round_gain_at_call_time(monkeypatch):
    M, n_out = 4096, 10240  # 16 x 40 = 640 e4m3 tiles -> 3 rounds x 256; bf16: 16 x 32 = 512 tiles -> 2 rounds x 320
    monkeypatch.setattr(U, "FP8_ROUND_GAIN", 1.3)
    assert U.fp8_geglu_pays(M, n_out) is True    # 768 < 1.3 * 640
    monkeypatch.setattr(U, "FP8_ROUND_GAIN", 1.0)
    assert U.fp8_geglu_pays(M, n_out) is False
    monkeypatch.setattr(U, "FP8_ROUND_GAIN", 1e9)
    assert U.fp8_geglu_pays(M, n_out) is True
