"""CPU: FilmSirenNeRF with hidden_layers other than 8 - the MI_FIELD_FILM_DEPTH kind ids through the size queries, the
Python modules, and the CPU restatement of the depth-L network against the reference-pinned fixtures
(tests/golden/make_golden_film_depth.py).  No compute call is made on the library."""
import ctypes

import numpy as np
import pytest
import torch

import film_depth_util as U
from mirender import _lib, fields, pigan

TOL_F4 = 2e-6          # the tolerance tests/test_oracle_golden.py uses for F4 (field outputs against the reference's)


def lib():
    return _lib.load()


@pytest.mark.parametrize("L", [4, 8, 12])
@pytest.mark.parametrize("use_dir", [True, False])
def test_size_queries_of_depth_kinds(L, use_dir):
    l, kind = lib(), U.kind_of(L, use_dir)
    spec = U.spec(L, use_dir)
    assert l.mi_field_num_params(kind) == 2 * (L + 3) == 2 * len(spec)
    rows, cols = ctypes.c_int64(), ctypes.c_int64()
    for i, (_, (o, c)) in enumerate(spec):
        assert l.mi_field_param_shape(kind, 2 * i, rows, cols) == 0 and (rows.value, cols.value) == (o, c)
        assert l.mi_field_param_shape(kind, 2 * i + 1, rows, cols) == 0 and (rows.value, cols.value) == (o, 1)
    assert l.mi_field_param_shape(kind, 2 * len(spec), rows, cols) == -1
    assert l.mi_field_macs(kind) == 256 * 3 + (L - 1) * 256 ** 2 + 256 + 256 * (259 if use_dir else 256) + 3 * 256
    assert l.mi_field_film_layers(kind) == L + 1
    assert l.mi_field_packed_floats(kind) % 256 == 0 and l.mi_field_packed_floats(kind) >= l.mi_field_macs(kind)
    assert l.mi_field_packed_bwd_floats(kind) % 256 == 0
    assert l.mi_field_train_acts_floats(kind) == 8 + 256 * (L + 1)
    assert l.mi_field_train_grads_floats(kind) == 256 * (L + 1) + 4
    assert fields.spec_of(fields.film_depth_kind(L, use_dir)) == spec
    assert fields.MACS[fields.film_depth_kind(L, use_dir)] == l.mi_field_macs(kind)


@pytest.mark.parametrize("use_dir", [True, False])
def test_depth_8_is_kinds_2_and_3(use_dir):
    l, a = lib(), U.kind_of(8, use_dir)
    b = fields.FILM_SIREN_NERF if use_dir else fields.FILM_SIREN_NERF_NODIR
    assert fields.film_depth_kind(8, use_dir) == b
    for q in ("mi_field_num_params", "mi_field_packed_floats", "mi_field_macs", "mi_field_film_layers",
              "mi_field_packed_bwd_floats", "mi_field_train_acts_floats", "mi_field_train_grads_floats"):
        assert getattr(l, q)(a) == getattr(l, q)(b) > 0, q
    assert l.mi_field_film_layers(b) == 9
    for pts in (100, 4096, 100000):
        assert l.mi_field_bwd_partial_floats_kind(a, pts) == l.mi_field_bwd_partial_floats_kind(b, pts) \
            == l.mi_field_bwd_partial_floats(pts)
    assert l.mi_field_film_partial_floats_kind(a, 2, 512) == l.mi_field_film_partial_floats_kind(b, 2, 512) \
        == l.mi_field_film_partial_floats(2, 512)
    assert l.mi_render_train_saved_bytes(a, a, 1, 64, 8, 16) == l.mi_render_train_saved_bytes(b, b, 1, 64, 8, 16)
    assert l.mi_render_backward_workspace_bytes(a, a, 1, 2, 32, 8, 16, 4096, 4096) \
        == l.mi_render_backward_workspace_bytes(b, b, 1, 2, 32, 8, 16, 4096, 4096)
    rows, cols, r2, c2 = (ctypes.c_int64() for _ in range(4))
    for i in range(22):
        assert l.mi_field_param_shape(a, i, rows, cols) == 0 == l.mi_field_param_shape(b, i, r2, c2)
        assert (rows.value, cols.value) == (r2.value, c2.value)


def test_non_film_kinds_have_no_film_rows():
    for kind in (fields.NERF, fields.SIREN_NERF, fields.TINY_NERF):
        assert lib().mi_field_film_layers(kind) == 0


@pytest.mark.parametrize("L", [3, 13])
def test_depth_out_of_range_is_refused_with_the_range(L):
    l = lib()
    for q in ("mi_field_num_params", "mi_field_packed_floats", "mi_field_film_layers", "mi_field_train_acts_floats"):
        assert getattr(l, q)(U.kind_of(L, True)) < 0
        msg = l.mi_last_error().decode()
        assert "4..12" in msg and str(L) in msg, msg
    assert l.mi_render_train_saved_bytes(U.kind_of(L, True), U.kind_of(L, True), 1, 64, 8, 16) < 0
    with pytest.raises(_lib.MiRenderError, match=r"4\.\.12"):
        fields.FilmSirenNeRF(hidden_layers=L)


@pytest.mark.parametrize("kind", [0x200 + 9, 0x1000, 77, -5])
def test_malformed_kind_id(kind):
    l = lib()
    assert l.mi_field_num_params(kind) < 0 and b"unknown field kind" in l.mi_last_error()
    assert l.mi_field_film_layers(kind) < 0


@pytest.mark.parametrize("use_dir", [True, False])
def test_depth_4_module_has_the_reference_layout(use_dir):
    m = fields.FilmSirenNeRF(hidden_layers=4, use_dir=use_dir)
    want = {}
    for key, (o, i) in U.spec(4, use_dir):
        want[key + ".weight"], want[key + ".bias"] = (o, i), (o,)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == want
    assert m.n_layers == 3 and m.use_dir is use_dir and isinstance(m, fields.FilmSirenNeRF)
    assert fields.detect_kind(dict(m.named_parameters())) == U.kind_of(4, use_dir) == m.KIND
    assert fields.hyper_mismatch(m, m.KIND) is None
    assert fields.is_film(m.KIND) and fields.film_layers(m.KIND) == 5
    # FilmSiren.reset_parameters (pi_GAN/modules.py:27-31): |w| <= sqrt(c / in) / w_0, first layer 1 / in
    assert float(m.hidden_layers[0].weight.abs().max()) <= np.sqrt(6 / 256) / 30 + 1e-9
    assert float(m.input_layer.weight.abs().max()) <= 1 / 3 + 1e-9


class _RefFilmSiren(torch.nn.Module):
    """A layer that says what the reference's FilmSiren says about itself: weight, bias, w_0."""

    def __init__(self, i, o, w_0=30):
        super().__init__()
        self.w_0 = w_0
        self.weight = torch.nn.Parameter(torch.zeros(o, i))
        self.bias = torch.nn.Parameter(torch.zeros(o))


class _RefLookAlike(torch.nn.Module):
    """The reference class's structure for hidden_layers = L (pi_GAN/modules.py:73-94), written out here."""

    def __init__(self, L, use_dir=True):
        super().__init__()
        self.input_layer = _RefFilmSiren(3, 256)
        self.hidden_layers = torch.nn.ModuleList([_RefFilmSiren(256, 256) for _ in range(L - 1)])
        self.output_layer_sigma = torch.nn.Sequential(torch.nn.Linear(256, 1), torch.nn.ReLU())
        self.hidden_layer_rgb = _RefFilmSiren(259 if use_dir else 256, 256)
        self.output_layer_rgb = torch.nn.Sequential(torch.nn.Linear(256, 3), torch.nn.Sigmoid())
        self.film_params = None


def test_reference_shaped_depth_4_is_recognised():
    m = _RefLookAlike(4)
    kind = fields.detect_kind(dict(m.named_parameters()))
    assert kind == U.kind_of(4, True)
    assert fields.hyper_mismatch(m, kind) is None
    assert fields.film_w0(m, kind) == 30.0
    # as_packed_field claims it; on a CPU-only host the claim ends at "needs a ROCm device", not at "unknown layout"
    if torch.cuda.is_available():
        assert fields.as_packed_field(m.cuda()) is not None
    else:
        with pytest.raises(_lib.MiRenderError, match="ROCm device"):
            fields.as_packed_field(m)
    assert fields.detect_kind(dict(_RefLookAlike(3).named_parameters())) is None


def test_other_widths_still_raise():
    with pytest.raises(_lib.MiRenderError):
        fields.FilmSirenNeRF(hidden_layers=4, hidden_dim=128)


def test_generator_depth_6():
    g = pigan.Generator(64, 16, hidden_layers=6)
    assert len(g.mapping_network.output_layers) == 7
    assert g.film_siren_nerf.KIND == U.kind_of(6, True) and len(g.film_siren_nerf.hidden_layers) == 5
    assert tuple(g.mapping_network(torch.zeros(2, 64)).shape) == (2, 7, 512)
    assert len(pigan.Generator(64, 16).mapping_network.output_layers) == 9        # the default is unchanged


def test_checkpoint_rebuilds_the_depth(tmp_path):
    from mirender import checkpoint
    g = pigan.Generator(32, 16, hidden_layers=5, use_dir=False)
    sd = {k: v.clone() for k, v in g.state_dict().items()}
    if torch.cuda.is_available():
        g2 = checkpoint.pigan_generator({"generator": sd}, 16)
        assert g2.film_siren_nerf.KIND == U.kind_of(5, False)
    m = fields.FilmSirenNeRF(hidden_layers=5, use_dir=False)
    m2 = fields.field_from_state_dict(m.state_dict(), device="cpu")
    assert m2.KIND == m.KIND and all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), m2.state_dict().values()))


@pytest.mark.parametrize("L", U.DEPTHS)
@pytest.mark.parametrize("use_dir", [True, False])
def test_restatement_reproduces_the_reference(golden, L, use_dir):
    g = golden(f"film_depth_L{L}_{'dir' if use_dir else 'nodir'}")
    film = U.film_rows(2, L, seed=100 + L)
    x = torch.from_numpy(g["x"])
    assert int(g["redraws"]) <= 25 and float(g["sigma_margin"]) >= 100
    for head in ("plain", "medium"):
        sd = U.state_dict(L, use_dir, seed=200 + L, head=head)
        assert U.digest(sd, film) == str(g[f"digest.{head}"]), "synthetic weights drifted from the fixture's"
        with torch.no_grad():
            out = U.forward(sd, film[1], x)
        assert float(np.abs(out.numpy().astype(np.float64) - g[f"out.{head}"]).max()) <= TOL_F4
    # the gradient call: the restatement's outputs and autograd against the reference's
    sd = U.state_dict(L, use_dir, seed=400 + L, head="medium")
    gfilm = U.film_rows(U.N_GROUPS, L, seed=500 + L)
    assert U.digest(sd, gfilm, U.grad_rays(), U.t_rand(), *U.cotangents()) == str(g["digest.grad"])
    outs, grads, g_film = U.oracle_render_grads(sd, gfilm)
    for name, o in zip(U.OUT_NAMES, outs):
        assert float(np.abs(o.numpy().astype(np.float64) - g[name]).max()) <= 1e-6, name
    for name, t in list(grads.items()) + [("film", g_film)]:
        flat = t.numpy().reshape(-1).astype(np.float64)
        l2 = float(g[f"g.{name}.l2"])
        assert float(np.abs(flat[g[f"g.{name}.idx"]] - g[f"g.{name}.val"]).max()) <= 1e-5 * l2, name
        assert abs(float(np.sqrt((flat ** 2).sum())) - l2) <= 1e-5 * l2, name
