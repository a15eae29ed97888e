"""The quality measurements of DESIGN.md §10.5, §11.5, §12.5 and §14.5 under a camera pairing, on the
CPU with the references: the frames and error measures of the four test_quality_* tests, computed with a chosen
path-tracer camera (`pt_camera`: the identity for the pairing before iqpt_camera_align, align_camera for the aligned
one) while the G-buffer keeps the plain camera, and a second figure restricted to the pixels within one pixel of an id
edge. The truth frame of a pairing is rendered with that pairing's own path-tracer camera."""
from __future__ import annotations

import numpy as np

import denoise_ref as dr
import iqpt
import oracle
import svgf_ref as sr
import temporal_ref as tr
import upscale_ref as ur
from iqpt import Scene, make_camera

NO = dr.NO_PRIM
W, H = 96, 54


def plain(cam):
    return cam


def edge_mask(ids):
    """Pixels whose 3 x 3 neighbourhood (clamped at the frame's border) holds another id."""
    h, w = ids.shape
    p = np.pad(ids, 1, mode="edge")
    m = np.zeros((h, w), bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            m |= p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w] != ids
    return m


def rmse(a, ref, mask):
    d = (a[..., :3].astype(np.float64) - ref)[mask]
    return float(np.sqrt(np.mean(d ** 2)))


def _scene():
    sc = Scene()
    sc.add_preset("cornell_lit")
    return sc, sc.build_packet(), sc.draw_list()


def denoise_figures(pt_camera):
    """test_denoise_ref.py::test_quality_on_the_oracle_frames: 4 spp filtered against 2048 spp."""
    sc, pk, items = _scene()
    cam = make_camera(W, H)
    fr = oracle.OracleFrame(W, H, max_depth=8, seed=1984)
    fr.render(pk, pt_camera(cam), 4)
    noisy = fr.lin.copy().reshape(H, W, 4)
    fr.render(pk, pt_camera(cam), 2044)
    ref = fr.lin.reshape(H, W, 4)[..., :3].astype(np.float64)
    nz, ids = dr.gbuffer_scene(items, cam, W, H)
    out, _ = dr.denoise(noisy, nz, ids, 3, 5, 1024.0, 2.0)
    every, edge = np.ones((H, W), bool), edge_mask(ids)
    return dict(raw=rmse(noisy, ref, every), out=rmse(out, ref, every), raw_edge=rmse(noisy, ref, edge),
                out_edge=rmse(out, ref, edge), edge_share=float(edge.mean()))


def history_figures(pt_camera):
    """test_temporal_ref.py and test_svgf_ref.py ::test_quality_on_the_oracle_frames: 8 views of 1 spp, the guided
    pixels of the last view against 1024 spp of another seed. Returns (temporal figures, svgf figures)."""
    sc, pk, items = _scene()
    fr = oracle.OracleFrame(W, H, max_depth=8, seed=1984)
    t = tr.Temporal(W, H, 0.9, 0.01, 256)
    p = iqpt.svgf.default_params()
    s = sr.Svgf(W, H, 0.9, 0.01, 256, p["min_history"], p["levels"], p["normal_squarings"], p["depth_sharpness"],
                p["colour_sigma"], p["variance_floor"])
    for k in range(8):
        cam = make_camera(W, H, position=[0.05 * k, 0.5, -3.0, 0.0], forward=[-0.02 * k, -0.5, 3.0, 0.0])
        nz, ids = dr.gbuffer_scene(items, cam, W, H)
        fr.reset()
        fr.render(pk, pt_camera(cam), 1)
        t.begin_view(cam, nz, ids)
        t_out, _ = t.resolve(fr.lin, 1)
        s.begin_view(cam, nz, ids)
        s_out, _ = s.resolve(fr.lin, 1)
    raw = fr.lin.copy().reshape(H, W, 4)
    guided = ids != NO
    truth = oracle.OracleFrame(W, H, max_depth=8, seed=77)
    truth.render(pk, pt_camera(cam), 1024)
    ref = truth.lin.reshape(H, W, 4)[..., :3].astype(np.float64)
    edge = edge_mask(ids) & guided

    def fig(out):
        return dict(raw=rmse(raw, ref, guided), out=rmse(out, ref, guided), raw_edge=rmse(raw, ref, edge),
                    out_edge=rmse(out, ref, edge), edge_share=float(edge.mean()))

    return fig(t_out), fig(s_out)


def upscale_figures(pt_camera):
    """test_upscale_ref.py::test_quality_and_classes_on_the_oracle_frames: lo 48x27 at 16 spp upsampled by 2 against the
    hi frame at 2048 spp (raw: the hi frame at 4 spp)."""
    f, w, h = 2, W // 2, H // 2
    sc, pk, items = _scene()
    cam_hi, cam_lo = make_camera(W, H), make_camera(w, h)
    fr = oracle.OracleFrame(W, H, max_depth=8, seed=1984)
    fr.render(pk, pt_camera(cam_hi), 4)
    noisy = fr.lin.copy().reshape(H, W, 4)
    fr.render(pk, pt_camera(cam_hi), 2044)
    ref = fr.lin.reshape(H, W, 4)[..., :3].astype(np.float64)
    lo = oracle.OracleFrame(w, h, max_depth=8, seed=1984)
    lo.render(pk, pt_camera(cam_lo), 16)
    lo16 = lo.lin.copy().reshape(h, w, 4)
    nz_hi, id_hi = dr.gbuffer_scene(items, cam_hi, W, H)
    nz_lo, id_lo = dr.gbuffer_scene(items, cam_lo, w, h)
    up16, _, _ = ur.upscale(lo16, nz_lo, id_lo, nz_hi, id_hi, f, 5, 1024.0)
    every, edge = np.ones((H, W), bool), edge_mask(id_hi)
    return dict(raw=rmse(noisy, ref, every), out=rmse(up16, ref, every), raw_edge=rmse(noisy, ref, edge),
                out_edge=rmse(up16, ref, edge), edge_share=float(edge.mean()))


def show(name, fig):
    return name + ": " + " ".join(f"{k} {v:.5f}" for k, v in fig.items())


if __name__ == "__main__":
    from iqpt import align_camera
    for pairing, pt_camera in (("one camera", plain), ("aligned", align_camera)):
        print(show(f"denoise, {pairing}", denoise_figures(pt_camera)))
        tf, sf = history_figures(pt_camera)
        print(show(f"temporal, {pairing}", tf))
        print(show(f"svgf, {pairing}", sf))
        print(show(f"upscale, {pairing}", upscale_figures(pt_camera)))
