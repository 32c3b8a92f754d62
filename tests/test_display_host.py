"""Host side of the display panels and the validation pass (no GPU): display.grid_shape, hand-built cases of the numpy restatement
(tests/display_restate.py) the device panel is checked against, and the argument checks of display / train_step.validate."""

import importlib

import numpy as np
import pytest
import torch

import display_restate as dr
from augment_restate import hsv180_to_rgb
from evaluate_restate import JET

ea = importlib.import_module("endoscopydepthestimation-pytorch_amd")
display = ea.display


@pytest.mark.parametrize("n, want", [(1, (64, 96)), (2, (68, 2 * 98 + 2)), (7, (68, 7 * 98 + 2)), (8, (68, 8 * 98 + 2)),
                                     (9, (2 * 66 + 2, 8 * 98 + 2)), (17, (3 * 66 + 2, 8 * 98 + 2))])
def test_grid_shape(n, want):
    assert display.grid_shape(n, 64, 96) == want
    assert dr.grid_shape(n, 64, 96) == want
    assert dr.make_grid(np.zeros((n, 1, 64, 96), np.float32)).shape == (1,) + want
    assert display.panel_shape(n, 64, 96) == (8 * want[0], want[1], 3)


def test_grid_shape_rejects_empty():
    for args in ((0, 4, 4), (2, 0, 4), (2, 4, -1)):
        with pytest.raises(ValueError):
            display.grid_shape(*args)


def test_make_grid_places_frames():
    """Frame k at row k // 8, column k % 8 of the grid, two pixels of padding around and between; cells past N stay padding."""
    n, h, w = 9, 3, 4
    frames = (np.arange(n, dtype=np.float32) + 1.0).reshape(n, 1, 1, 1) * np.ones((n, 1, h, w), np.float32)
    g = dr.make_grid(frames)[0]
    assert g.shape == (2 * (h + 2) + 2, 8 * (w + 2) + 2)
    for k in range(n):
        y, x = divmod(k, 8)
        cell = g[y * (h + 2) + 2:y * (h + 2) + 2 + h, x * (w + 2) + 2:x * (w + 2) + 2 + w]
        assert np.all(cell == k + 1)
    assert np.count_nonzero(g) == n * h * w
    one = dr.make_grid(frames[:1])
    assert one.shape == (1, h, w) and np.all(one == 1.0)


def test_padding_is_jet0_in_depth_rows_and_black_in_flow_rows():
    rng = np.random.default_rng(0)
    n, h, w = 3, 5, 6
    depth = rng.uniform(1.0, 2.0, (n, 1, h, w)).astype(np.float32)
    b = np.ones((n, 1, h, w), np.float32)
    d = dr.depth_section(depth, b)
    pad = np.ones(d.shape[:2], bool)
    for k in range(n):
        pad[2:2 + h, 2 + k * (w + 2):2 + k * (w + 2) + w] = False
    assert np.all(d[pad] == JET[0][::-1])
    flows = rng.standard_normal((n, 2, h, w)).astype(np.float32)
    f, top = dr.flow_section(flows)
    assert top > 0 and np.all(f[pad] == 0)
    assert np.count_nonzero(f[~pad].any(axis=-1)) > 0


def test_constant_depth_frame_is_jet0():
    depth = np.full((2, 1, 4, 5), 3.25, np.float32)
    depth[1] = np.linspace(1.0, 2.0, 20, dtype=np.float32).reshape(1, 4, 5)
    d = dr.depth_section(depth, np.ones_like(depth))
    assert np.all(d[2:6, 2:7] == JET[0][::-1])
    second = d[2:6, 9:14]
    assert np.array_equal(second[0, 0], JET[0][::-1]) and np.array_equal(second[-1, -1], JET[254][::-1])          # 255 (1 - 1e-5 / 1) truncates to 254


def test_zero_sparse_flows_render_black():
    """max_v = np.max(v) = 0: v / max_v is 0 / 0 = NaN, which the reference's np.uint8 turns into V = 0 -- black; the dense flows reuse that
    max_v, so their non-zero pixels divide to +inf and saturate (V = 255), their zero pixels are black."""
    sparse = np.zeros((1, 2, 4, 4), np.float32)
    rgb, top = dr.flow_section(sparse)
    assert top == 0 and np.all(rgb == 0)
    dense = np.zeros((1, 2, 4, 4), np.float32)
    dense[0, 0, 1, 1] = 0.5
    hsv, _ = dr.flow_hsv(dense, max_v=top)
    assert hsv[1, 1, 2] == 255 and hsv[0, 0, 2] == 0


def test_unit_x_flow_is_hue_90():
    """fx = 1, fy = 0: arctan2(0, 1) + pi = pi, times 180 / pi / 2 in float32 is 90.000..., truncated to 90 -- cyan after HSV -> RGB."""
    flows = np.zeros((1, 2, 2, 3), np.float32)
    flows[0, 0] = 1.0
    hsv, top = dr.flow_hsv(flows)
    assert top == 1.0 and np.all(hsv[..., 0] == 90) and np.all(hsv[..., 2] == 255)
    literal, _ = dr.flow_hsv(flows, literal=True)
    assert np.array_equal(literal, hsv)
    rgb, _ = dr.flow_section(flows)
    assert np.all(rgb == hsv180_to_rgb(np.array([90, 255, 255], np.uint8)))
    assert np.array_equal(hsv180_to_rgb(np.array([90, 255, 255], np.uint8)), [0, 255, 255])


def test_flow_y_uses_the_grid_aspect():
    """draw_flow scales fy by the GRID's height / width: for N = 2 frames of 4 x 4 the grid is 8 x 14, so (0, 1) becomes (0, 8 / 14)."""
    flows = np.zeros((2, 2, 4, 4), np.float32)
    flows[:, 1] = 1.0
    hsv, top = dr.flow_hsv(flows)
    assert top == np.float32(np.float32(8) / np.float32(14))
    angle = np.float32(np.pi / 2) + np.float32(np.pi)
    assert hsv[2, 2, 0] == int(angle * np.float32(180 / np.pi / 2))


def test_colour_section_truncates():
    c = np.array([-1.0, 0.0, 1.0, np.float32(2 * 100 / 255.0 - 1.0)], np.float32).reshape(1, 1, 1, 4) * np.ones((1, 3, 1, 1), np.float32)
    u = dr.color_section(c)
    assert u.shape == (1, 4, 3)
    want = (np.float32(255) * (np.float32(0.5) * c[0, 0, 0] + np.float32(0.5))).astype(np.uint8)
    assert np.array_equal(u[0, :, 0], want) and list(u[0, :3, 1]) == [0, 127, 255]


def test_panel_stacks_eight_sections():
    rng = np.random.default_rng(3)
    n, h, w = 2, 4, 5
    c = rng.uniform(-1, 1, (2, n, 3, h, w)).astype(np.float32)
    d = rng.uniform(1, 2, (2, n, 1, h, w)).astype(np.float32)
    b = np.ones((n, 1, h, w), np.float32)
    f = rng.standard_normal((4, n, 2, h, w)).astype(np.float32)
    p = dr.panel(c[0], c[1], d[0], d[1], b, f[0], f[1], f[2], f[3])
    gh, gw = dr.grid_shape(n, h, w)
    assert p.shape == (8 * gh, gw, 3) and p.dtype == np.uint8
    assert np.array_equal(p[:gh], dr.color_section(c[0])) and np.array_equal(p[5 * gh:6 * gh], dr.depth_section(d[1], b))
    sf2, top2 = dr.flow_section(f[1])
    assert np.array_equal(p[6 * gh:7 * gh], sf2) and np.array_equal(p[7 * gh:], dr.flow_section(f[3], max_v=top2)[0])


def test_panels_argument_errors():
    x = torch.zeros((1, 3, 4, 4))
    with pytest.raises(NotImplementedError):
        display.panels(x, x, x, x, x, x, x, x, x, is_hsv=True)
    one = torch.zeros((1, 1, 4, 4))
    two = torch.zeros((1, 2, 4, 4))
    with pytest.raises(ValueError):          # host tensors: the panel is rendered on the device only
        display.panels(x, x, one, one, one, two, two, two, two)
    with pytest.raises(ValueError):
        display.panels(torch.zeros((1, 2, 4, 4)), x, one, one, one, two, two, two, two)


def test_stack_and_display_calls_the_writer():
    calls = []

    class Writer(object):
        def add_image(self, tag, img, step):
            calls.append((tag, img, step))
    panel = torch.arange(2 * 5 * 3, dtype=torch.uint8).reshape(2, 5, 3)
    display.stack_and_display("Validation", "Results (c1, d1, sf1, df1, c2, d2, sf2, df2)", 7, Writer(), panel)
    ((tag, img, step),) = calls
    assert tag == "Validation/Images/Results (c1, d1, sf1, df1, c2, d2, sf2, df2)" and step == 7
    assert img.shape == (3, 2, 5) and img.dtype == np.uint8 and np.array_equal(img, panel.numpy().transpose(2, 0, 1))
    with pytest.raises(ValueError):
        display.stack_and_display("Training", "t", 0, Writer(), panel.float())


def test_validate_argument_errors():
    class Step(object):
        fused_head = True
    for kw in (dict(display_each=0, on_display=lambda i, p: None), dict(display_each=-3, on_display=lambda i, p: None),
               dict(display_each=2), dict(on_display=lambda i, p: None), dict(initial=(1.0, 2.0))):
        with pytest.raises(ValueError):
            ea.train_step.validate(Step(), [], **kw)
    Step.fused_head = False
    with pytest.raises(ValueError, match="fused"):
        ea.train_step.validate(Step(), [], display_each=1, on_display=lambda i, p: None)
    empty = ea.train_step.validate(Step(), [], initial=(1.0, 2.0, 3.0))
    assert (empty.mean_loss, empty.mean_depth_consistency_loss, empty.mean_sparse_flow_loss) == (1.0, 2.0, 3.0)
    assert empty.running_means.shape == (0, 3) and empty.losses.shape == (0, 3)
    nan = ea.train_step.validate(Step(), [])
    assert all(np.isnan(v) for v in nan[:3])
