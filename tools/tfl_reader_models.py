"""Writes the per-channel int8 models of the reader's CPU test (tests/tfl_models_q.reader_models) as .tflite files into a directory,
for the stand-alone sanitizer program tools/tfl_reader_check.cpp.   usage: tfl_reader_models.py DIR"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tfl_builder_q as BQ, tfl_models_q as MQ
os.makedirs(sys.argv[1], exist_ok=True)
for i, m in enumerate(MQ.reader_models()):
    path = os.path.join(sys.argv[1], "per_channel_%d.tflite" % i)
    open(path, "wb").write(BQ.serialize(m))
    print(path)
