"""Training entry points (reference: lib/detect/train_az.py).  Only the roidb side exists here: the solver, the
losses and the backward pass are not part of this backend yet."""
import az_data_layer.roidb as rdl_roidb
from detect.config import cfg


def get_training_roidb(imdb):
    """A roidb for use in training (train_az.py:118-129)."""
    if cfg.TRAIN.USE_FLIPPED:
        print("Appending horizontally-flipped training examples...")
        imdb.append_flipped_images()
        print("done")
    print("Preparing training data...")
    rdl_roidb.prepare_roidb(imdb)
    print("done")
    return imdb.roidb
