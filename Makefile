# Builds libspectral.so (gfx950 only) in-tree so it travels to the GPU box with the snapshot.
HIPCC   ?= /opt/rocm/bin/hipcc
ARCH    ?= gfx950
CSRC    := pyfft_amd/csrc
LIBDIR  := pyfft_amd/lib
OBJDIR  := build/obj
FLAGS   := -O3 -std=c++17 -fPIC -fno-slp-vectorize --offload-arch=$(ARCH) -Iinclude -I$(CSRC) -Wall -Wno-unused-function

SRCS    := $(wildcard $(CSRC)/*.hip)
OBJS    := $(patsubst $(CSRC)/%.hip,$(OBJDIR)/%.o,$(SRCS))
HDRS    := $(wildcard $(CSRC)/*.h) include/spectral.h include/spectral_ext.h include/spectral_tfr.h include/spectral_quad.h include/spectral_cyclo.h include/spectral_uneven.h include/spectral_wbic.h include/spectral_fam.h include/spectral_nufft.h include/spectral_nufft2.h include/spectral_ar.h include/spectral_sub.h include/spectral_dwt.h include/spectral_array.h include/spectral_mimo.h

all: $(LIBDIR)/libspectral.so

$(OBJDIR)/%.o: $(CSRC)/%.hip $(HDRS) Makefile
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(FLAGS) -c $< -o $@

$(LIBDIR)/libspectral.so: $(OBJS)
	@mkdir -p $(LIBDIR)
	$(HIPCC) -shared -fPIC --offload-arch=$(ARCH) $(OBJS) -o $@

clean:
	rm -rf build $(LIBDIR)/libspectral.so

.PHONY: all clean
