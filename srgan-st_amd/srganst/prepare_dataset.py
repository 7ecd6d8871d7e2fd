"""Cut a directory of whole images into square HR tiles - the offline route of the reference's data-prep/prepare_dataset.py
(:27-47), without cv2: every image of --input_dir that is at least --output_size on both sides is cut on the grid
y in range(0, H - size + 1, step), x in range(0, W - size + 1, step), row-major, and tile number `index` (from 1) is written as
`{name}_{index:04d}.{ext}` into --output_dir, where name / ext are the second-to-last / last dot-separated parts of the file name,
as the reference forms them.  The tiles keep the image's mode and file format (PIL).

    python -m srganst.prepare_dataset --input_dir DIV2K_train_HR --output_dir data/train --output_size 96 --step_size 96

The grid is device_data.tile_grid, the one DATA.ON_DEVICE_WHOLE_IMAGES walks on the device without writing any file.
"""
from __future__ import annotations

import argparse
import os
from concurrent.futures import ThreadPoolExecutor


def tile_name(image_file_name: str, index: int) -> str:
    parts = image_file_name.split(".")
    return f"{parts[-2]}_{index:04d}.{parts[-1]}"


def cut_image(input_dir: str, output_dir: str, image_file_name: str, output_size: int, step_size: int) -> int:
    """Writes the tiles of one image; returns how many."""
    from PIL import Image
    from .device_data import tile_grid
    with Image.open(os.path.join(input_dir, image_file_name)) as im:
        im.load()
        w, h = im.size
        tiles = tile_grid([(h, w)], output_size, step_size)
        for index, (_, y, x) in enumerate(tiles.tolist(), start=1):
            im.crop((x, y, x + output_size, y + output_size)).save(os.path.join(output_dir, tile_name(image_file_name, index)))
    return len(tiles)


def prepare(input_dir: str, output_dir: str, output_size: int = 96, step_size: int = 96, num_workers: int = 16) -> int:
    """Cuts every file of `input_dir`; returns the number of tiles written."""
    if output_size <= 0 or step_size <= 0:
        raise ValueError(f"prepare_dataset: output_size {output_size} and step_size {step_size} must be positive")
    os.makedirs(output_dir, exist_ok=True)
    names = os.listdir(input_dir)
    with ThreadPoolExecutor(max(1, num_workers)) as pool:
        return sum(pool.map(lambda n: cut_image(input_dir, output_dir, n, output_size, step_size), names))


def main(argv=None) -> None:
    ap = argparse.ArgumentParser(description="Cut a directory of images into square HR tiles (the training crops).")
    ap.add_argument("--input_dir", type=str, default="/work3/s204163/data/original")
    ap.add_argument("--output_dir", type=str, default="/work3/s204163/data/train")
    ap.add_argument("--output_size", type=int, default=96)
    ap.add_argument("--step_size", type=int, default=96)
    ap.add_argument("--num_workers", type=int, default=16)
    a = ap.parse_args(argv)
    n = prepare(a.input_dir, a.output_dir, a.output_size, a.step_size, a.num_workers)
    print(f"{n} tiles of {a.output_size} px written to {a.output_dir}")


if __name__ == "__main__":
    main()
