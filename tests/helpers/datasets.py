"""Synthetic datasets the driver tests share."""
import json

import numpy as np


def pie_dataset(tmp_path):
    """three PIE-Bench-style entries (categories 0, 1, 7) under tmp_path/data: annotation_images/ + mapping_file.json"""
    from PIL import Image
    d = tmp_path / "data"
    (d / "annotation_images" / "0_random").mkdir(parents=True)
    y, x = np.mgrid[0:96, 0:128]
    mapping = {}
    for i, (src, tar, blend, cat) in enumerate([("a cat sitting on a bench", "a dog sitting on a bench", "cat dog", "0"),
                                                 ("a [red] car", "a [blue] car on a road", "", "1"),
                                                 ("a tree", "a tall tree", "tree tree", "7")]):
        img = np.stack([(x * (i + 2)) % 256, (y * 3 + i * 40) % 256, (x + y) % 256], -1).astype(np.uint8)
        rel = f"0_random/{i:012d}.png"
        Image.fromarray(img).save(d / "annotation_images" / rel)
        mapping[f"{i:012d}"] = dict(image_path=rel, original_prompt=src, editing_prompt=tar, editing_instruction="",
                                    editing_type_id=cat, blended_word=blend)
    with open(d / "mapping_file.json", "w") as f:
        json.dump(mapping, f)
    return d
