"""Plug-in helpers that configurations name (mirror of neuralmonkey/util): ``word2vec``."""
