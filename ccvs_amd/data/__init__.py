"""Real clips from frame folders (the reference's `data/` package for the frame-folder datasets, validation phase): discovery,
clip choice and transform geometry on the host, crop / Pillow-exact resample / normalise on the GPU (`ops.ingest_u8`).
DESIGN.md section 4.14 says what is pinned against Pillow itself and what by restatement of the reference.  The datasets of video
files (ucf101, drums, kinetics600) are read from Motion-JPEG AVI: `VideoDataset` / `VideoLoader`, section 4.17."""
from .folder_dataset import IMG_EXTENSIONS, NPY_EXTENSION, make_dataset   # noqa: F401
from .frame_dataset import FrameDataset, FrameLoader, frames_root   # noqa: F401
from .video_dataset import VideoDataset, VideoLoader   # noqa: F401
