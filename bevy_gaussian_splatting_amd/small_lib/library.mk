# The one build recipe of the small device libraries (csrc_query/, csrc_sparse/, csrc_slice/, csrc_morph/). Each one's
# Makefile states LIB (the library's name), BUILD_ID_MACRO, SRCS and HDRS and includes this file; `make` runs in that
# library's directory, so every path here is relative to it. hipcc cross-compiles without a GPU. A library links the HIP
# runtime only: not libbgs, not another small library.
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
PYTHON ?= python3
# The flags of ../csrc/Makefile, for its reasons, and the same line (tests/test_native_binding.py compares them):
# -ffp-contract=off because every small library is compared bit for bit with its numpy twin, -fno-slp-vectorize because
# a packed f32 instruction gains nothing per operation on this chip. Nothing here relaxes f32 division or square root.
HIPFLAGS ?= --offload-arch=$(ARCH) -O3 -std=c++17 -ffp-contract=off -fno-slp-vectorize -fPIC -Wall -Wno-unused-function
# host code every *_api.hip includes; part of each library's hash, as this file is (../_build_id.py)
SHARED = ../small_lib/library.mk ../small_lib/api_support.h ../small_lib/api_support_hip.h

all: $(LIB).so
# The SHA-256 of the sources (../_build_id.py $(LIB)), compiled into the library as the byte string $(BUILD_ID_MACRO)=<hex>.
# Regenerated on every make, rewritten only when the hash changed; the library depends on it, so a source change
# rebuilds it whatever the files' mtimes say. One compile-and-link step: no object files are kept.
.PHONY: all clean FORCE
build_id.inc: FORCE
	@id=$$($(PYTHON) ../_build_id.py $(LIB)) && \
	 if [ "$$(cat $@ 2>/dev/null)" != "#define $(BUILD_ID_MACRO) \"$$id\"" ]; then echo "#define $(BUILD_ID_MACRO) \"$$id\"" > $@; fi
FORCE:
$(LIB).so: $(SRCS) $(HDRS) $(SHARED) build_id.inc
	$(HIPCC) $(HIPFLAGS) -shared -Wl,--version-script=$(LIB).map -o $@ $(SRCS)
clean:
	rm -f $(LIB).so build_id.inc
