"""run.py --shader with an effect added after Fog and Toon: the CLI accepts it and writes the GPU
effect of the plain frame, with run.py:248's depth normalisation."""
import os

import numpy as np
import pytest

import run as cli


@pytest.mark.gpu
def test_render_with_pencil_sketch(tmp_path):
    from PIL import Image
    from nerfmi.post_processor import PostProcessor, normalize_depth
    base = ["--mode", "render", "--random_init", "0", "--frames", "1", "--quality", "preview", "--width", "32",
            "--height", "32"]
    plain, sketch = str(tmp_path / "plain"), str(tmp_path / "sketch")
    assert cli.main(base + ["--output_dir", plain, "--save_depth"]) == 0
    assert cli.main(base + ["--output_dir", sketch, "--shader", "Pencil Sketch"]) == 0
    img = np.array(Image.open(os.path.join(plain, "rgb_000.png")))
    depth = np.load(os.path.join(plain, "raw", "depth_000.npy"))
    pp = PostProcessor()
    pp.current_effect = "Pencil Sketch"
    exp = pp.apply_effect(img, normalize_depth(depth))
    got = np.array(Image.open(os.path.join(sketch, "rgb_000.png")))
    assert got.shape == (32, 32, 3) and np.array_equal(got, exp)
    assert not np.array_equal(got, img)
