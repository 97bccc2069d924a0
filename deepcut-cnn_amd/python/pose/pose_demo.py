#!/usr/bin/env python
"""Command-line demo with the reference's flags (python/pose/pose_demo.py:45-74): predict the pose of an
image (or of every image in a folder), write `<image>_pose.npz` (key `pose`, 5x14) and optionally a PNG
overlay.  Needs an MI355X: `--use_cpu` is refused, this package has no CPU forward path."""
import glob
import logging
import os
import sys

import click
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(_HERE))  # .../python: `caffe`, `pose`, `deepcut_tools`

from pose.estimate_pose import estimate_pose  # noqa: E402

LOG = logging.getLogger(__name__)
COLORS = [[255, 0, 0], [0, 255, 0], [0, 0, 255], [0, 245, 255], [255, 131, 250], [255, 255, 0]] * 2 + [[0, 0, 0], [255, 255, 255]]


def draw_disc(image, cx, cy, radius, color):
    h, w = image.shape[:2]
    yy, xx = np.ogrid[:h, :w]
    image[(xx - int(cx)) ** 2 + (yy - int(cy)) ** 2 <= radius ** 2] = color


@click.command()
@click.argument("image_name", type=click.Path(exists=True, dir_okay=True, readable=True))
@click.option("--out_name", type=click.Path(dir_okay=True, writable=True), default=None)
@click.option("--scales", type=click.STRING, default="1.")
@click.option("--visualize", type=click.BOOL, default=True)
@click.option("--folder_image_suffix", type=click.STRING, default=".png")
@click.option("--use_cpu", type=click.BOOL, is_flag=True, default=False)
@click.option("--gpu", type=click.INT, default=0)
@click.option("--tiling", type=click.Choice(["none", "exact", "reference"]), default="none",
              help="none: one forward per scale (default); exact / reference: see pose.estimate_pose")
@click.option("--skeleton", type=click.BOOL, is_flag=True, default=False,
              help="draw the overlay on the device: joints and the MPII limbs, coloured by joint (pose.draw_people); default: discs only")
@click.option("--heatmap", type=click.Choice(["max", "joints"]), default=None,
              help="also write <out>_heat.png: the score maps of one forward at the first scale blended over the image on the device "
                   "(Net.draw_heatmap) — max: the maximum over the joints through caffe.HEAT_LUT; joints: every joint in its colour; default: off")
@click.option("--redact", type=click.Choice(["head", "body"]), default=None,
              help="pixelate the person's head or whole body in the visualisation on the device, under the overlay (pose.redact_people; "
                   "its radii are placeholders, and a mosaic is not a privacy guarantee); default: off")
@click.option("--labels", type=click.BOOL, is_flag=True, default=False,
              help="write the person's number over the visualisation on the device (pose.label_people): this demo has no tracker, so it "
                   "is the person's index — pose.track_people(labels=True) writes a tracker's ids; default: off")
@click.option("--model_def", default=None,
              help="model definition (.prototxt).  Default: the definition deepcut_tools.deepercut_prototxt(152) generates, which is "
                   "layer-for-layer the reference's models/deepercut/ResNet-152.prototxt (that directory is not part of this repository)")
@click.option("--model_bin", default=None, required=True,
              help="trained weights (.caffemodel / .h5): the reference fetches them with models/deepercut/download_models.sh; not shipped here")
def predict_pose_from(image_name, out_name, scales, visualize, folder_image_suffix, use_cpu, gpu, tiling, skeleton, heatmap, redact, labels, model_def, model_bin):
    import caffe
    from PIL import Image

    if model_def is None:
        import tempfile

        from deepcut_tools import deepercut_prototxt

        fd, model_def = tempfile.mkstemp(suffix=".prototxt")
        with os.fdopen(fd, "w") as f:
            f.write(deepercut_prototxt(152))

    scales = [float(v) for v in scales.split(",")]
    if os.path.isdir(image_name):
        images = sorted(glob.glob(os.path.join(image_name, "*" + folder_image_suffix)))
        folder = True
    else:
        images, folder = [image_name], False
    if use_cpu:
        caffe.set_mode_cpu()  # forward() will raise: there is no CPU path in libdeepcut_hip
    else:
        caffe.set_mode_gpu()
        caffe.set_device(gpu)
    if folder and out_name is not None and not os.path.exists(out_name):
        os.mkdir(out_name)
    for path in images:
        target = (path + "_pose.npz") if out_name is None else (
            os.path.join(out_name, os.path.basename(path) + "_pose.npz") if folder else out_name)
        img = np.asarray(Image.open(path))
        if img.ndim == 2:
            LOG.warning("The image is grayscale! This may deteriorate performance!")
            img = np.dstack((img, img, img))
        img = img[:, :, :3][:, :, ::-1]  # RGB -> BGR
        pose = estimate_pose(img, model_def, model_bin, scales, tiling=None if tiling == "none" else tiling)
        np.savez_compressed(target, pose=pose)
        if visualize and pose is not None and redact is not None:
            from pose.people import redact_people

            img = np.ascontiguousarray(img)
            redact_people(img, np.ascontiguousarray(pose[:3].T)[None], region=redact)
        if visualize and pose is not None and skeleton:
            from pose.people import SKELETON_MPII14, draw_people

            bgr = np.ascontiguousarray(img)
            draw_people(bgr, np.ascontiguousarray(pose[:3].T)[None], edges=SKELETON_MPII14, color="joint", joint_radius=8.0, limb_radius=3.0)
            if labels:
                from pose.people import label_people

                label_people(bgr, np.ascontiguousarray(pose[:3].T)[None])
            vis = bgr[:, :, ::-1]
            Image.fromarray(np.ascontiguousarray(vis)).save(target + "_vis.png")
        elif visualize and pose is not None:
            vis = img[:, :, ::-1].copy()
            for j in range(14):
                draw_disc(vis, pose[0, j], pose[1, j], 8, COLORS[j])
            if labels:
                from pose.people import label_people

                bgr = np.ascontiguousarray(vis[:, :, ::-1])
                label_people(bgr, np.ascontiguousarray(pose[:3].T)[None])
                vis = np.ascontiguousarray(bgr[:, :, ::-1])
            Image.fromarray(vis).save(target + "_vis.png")
        if heatmap is not None:
            from pose.estimate_pose import _get_model

            net = _get_model(model_def, model_bin)
            bgr = np.ascontiguousarray(img)
            net.forward_images(bgr, scales[0], want=(), pose=False)
            net.draw_heatmap(bgr, scales[0], mode=heatmap, alpha=192 if heatmap == "max" else 256, min_score=0.1)
            Image.fromarray(np.ascontiguousarray(bgr[:, :, ::-1])).save(target + "_heat.png")


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO)
    predict_pose_from()  # pylint: disable=no-value-for-parameter
