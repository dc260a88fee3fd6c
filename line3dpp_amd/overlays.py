"""A dataset's 3D lines drawn over its own images: one of the front-end programs (front_end.py), then one PNG per view.

    python -m line3dpp_amd.overlays <vsfm|colmap|bundler|pix4d|openmvg|mavmap> <that program's flags>
                                    [--views id,id,...] [--thickness n] [--alpha a]

runs the program exactly as `python -m line3dpp_amd.front_end` does -- same flags, same result files -- with a `Line3D`
whose `addImages` keeps the images of the selected views as they are handed to the library (undistorted), and then
writes <output_folder>/overlays/<camID>.png: the reconstructed lines of `Line3D.drawLines` over each kept
image, one colour per 3D line.

    --views id,id,...   camera ids to draw (as the program passes them to addImage); default: every view that was
                        added, which holds every image of the dataset in host memory until the end of the run
    --thickness n       width of the drawn lines in pixels, odd (default 1)
    --alpha a           opacity of the lines, 0 ... 255 (default 255)
"""
import os
import sys

from . import front_end
from .api import Line3D

CHUNK_BYTES = 256 << 20     # RGB output of one drawLines call at most (a view more than this goes alone)
OWN_FLAGS = {"--views": "views", "--thickness": "thickness", "--alpha": "alpha"}


def split_args(argv):
    """-> (the front end's own arguments, dict of this program's three flags); raises ValueError on a bad value"""
    rest, own = [], dict(views=None, thickness=1, alpha=255)
    i = 0
    while i < len(argv):
        name, eq, value = argv[i].partition("=")
        if name in OWN_FLAGS:
            if not eq:
                if i + 1 >= len(argv):
                    raise ValueError(f"{name} needs a value")
                i += 1
                value = argv[i]
            own[OWN_FLAGS[name]] = [int(v) for v in value.split(",") if v] if name == "--views" else int(value)
        else:
            rest.append(argv[i])
        i += 1
    return rest, own


def keeping_line3d(views):
    """a Line3D class whose addImages keeps the images of `views` (None: all) that were added: .kept = {camID: image}"""
    class KeepingLine3D(Line3D):
        def __init__(self, *args, **kwargs):
            super().__init__(*args, **kwargs)
            self.kept = {}

        def addImages(self, camIDs, images, Ks, Rs, ts, median_depths, wps_or_neighbors):
            camIDs, images = [int(c) for c in camIDs], list(images)
            super().addImages(camIDs, images, Ks, Rs, ts, median_depths, wps_or_neighbors)
            for cam, image in zip(camIDs, images):
                if cam in self._M and cam not in self.kept and (views is None or cam in views):
                    self.kept[cam] = image
    return KeepingLine3D


def write_overlays(line3d, thickness=1, alpha=255, chunk_bytes=None):
    """<output_folder>/overlays/<camID>.png for every kept image, one drawLines call per chunk of views -> the paths"""
    from PIL import Image
    folder = os.path.join(line3d.output_folder, "overlays")
    os.makedirs(folder, exist_ok=True)
    budget = CHUNK_BYTES if chunk_bytes is None else chunk_bytes
    cams, paths = sorted(line3d.kept), []
    while cams:
        chunk, held = [], 0
        while cams and (not chunk or held + 3 * line3d.kept[cams[0]].size <= budget):
            held += 3 * line3d.kept[cams[0]].size
            chunk.append(cams.pop(0))
        drawn = line3d.drawLines(chunk, [line3d.kept[c] for c in chunk], thickness, alpha)
        if drawn is None:
            raise front_end.FrontEndError("drawLines failed", 4)
        for cam, rgb in zip(chunk, drawn):
            paths.append(os.path.join(folder, f"{cam}.png"))
            Image.fromarray(rgb, "RGB").save(paths[-1])
    return paths


def main(argv=None):
    """the program: -> exit status"""
    argv = list(sys.argv[1:] if argv is None else argv)
    if not argv or argv[0] not in front_end.PROGRAMS:
        print(__doc__, file=sys.stderr)
        return 1
    try:
        rest, own = split_args(argv[1:])
    except ValueError as e:
        print(f"{e}\n\n{__doc__}", file=sys.stderr)
        return 1
    views = None if own["views"] is None else set(own["views"])
    try:
        line3d, times = front_end.PROGRAMS[argv[0]](rest, line3d_factory=keeping_line3d(views))
        paths = write_overlays(line3d, own["thickness"], own["alpha"])
    except front_end.FrontEndError as e:
        print(e, file=sys.stderr)
        if isinstance(e, front_end.UsageError):
            print("\n" + front_end.usage(argv[0]), file=sys.stderr)
        return e.status
    if views is not None and views - set(line3d.kept):
        print(f"{front_end.PREFIX}WARNING: no such view was added: {sorted(views - set(line3d.kept))}")
    print(f"{front_end.PREFIX}{len(paths)} overlays written to {os.path.join(line3d.output_folder, 'overlays')}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
