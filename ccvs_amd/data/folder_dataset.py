"""Frame discovery (reference data/folder_dataset.py:7-57).

One extension of ours: a frame may also be a `.npy` file holding uint8 [H, W, 3] (RGB), so that a dataset can exist -- and the
loader be tested -- where no image codec is installed."""
import os

IMG_EXTENSIONS = ['.jpg', '.JPG', '.jpeg', '.JPEG', '.png', '.PNG', '.ppm', '.PPM', '.bmp', '.BMP', '.tiff', '.webp']
NPY_EXTENSION = '.npy'
VID_EXTENSIONS = ['.avi', '.mp4']


def is_img_file(filename):
    return any(filename.endswith(ext) for ext in IMG_EXTENSIONS) or filename.endswith(NPY_EXTENSION)


def is_vid_file(filename):
    return any(filename.endswith(ext) for ext in VID_EXTENSIONS)


def make_dataset(dir, recursive=True, from_vid=False):
    """Paths of every frame (from_vid: of every video file, folder_dataset.py:8,16-17) under `dir`: `os.walk(dir, followlinks=True)` with the directories in sorted order
    (folder_dataset.py:19-26).  The reference takes the files of one directory in the file system's order; here they are sorted, so
    that the list is the same on every machine (the grouping into videos sorts the paths anyway, bairhd_dataset.py:25)."""
    if not os.path.isdir(dir):
        raise FileNotFoundError(f"{dir} is not a valid directory")
    files = []
    for root, _, fnames in sorted(os.walk(dir, followlinks=recursive)):
        for fname in sorted(fnames):
            if (is_vid_file(fname) if from_vid else is_img_file(fname)):
                files.append(os.path.join(root, fname))
        if not recursive:
            break
    return files
