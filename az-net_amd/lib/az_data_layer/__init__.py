"""The AZ-net training data layer (reference: lib/az_data_layer): the trainable roidb -- example regions, zoom labels
and adjacency targets, built on the GPU (csrc/az_train.hip) -- and the minibatch sampler over it."""
