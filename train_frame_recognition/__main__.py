"""python -m train_frame_recognition --config cfg.yaml: the command line of the frame-classifier trainer (see the package)."""
from artspeech_amd.training import run_cli

from . import main

if __name__ == "__main__":
    run_cli(main, "frame_recognition")
