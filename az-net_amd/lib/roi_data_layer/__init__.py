"""The detection net's training data layer (reference: lib/roi_data_layer): the trainable roidb -- the AZ-net's proposals
stacked on the ground truth, box-regression targets and their per-class normalisation built on the GPU
(csrc/az_det_train.hip) -- and the minibatch sampler over it."""
