# lib.mk -- the one build rule of the image-side libraries.  A library's Makefile sets NAME (and EXTRA_DEPS, if it has more
# prerequisites) and includes this file from its own directory: ../NAME_csrc/pc_NAME.hip + pc_NAME.h -> ../libpc_NAME.so, gfx950 only.
# Every library is linked on its own and links no other library of the project; what they share is the headers of this directory,
# which are prerequisites of every object: editing one rebuilds all ten.
# -ffp-contract=off as everywhere: every fused multiply-add is an explicit fmaf (the contracts are stated in single IEEE operations).
HIPCC   ?= /opt/rocm/bin/hipcc
ARCH    ?= gfx950
FLAGS   ?= -O3 -std=c++17 -fPIC -ffp-contract=off -fvisibility=hidden --offload-arch=$(ARCH) -Wall -Wno-unused-function
OUT     := ../libpc_$(NAME).so
SHARED  := $(wildcard ../image_csrc/*.h)

all: $(OUT)

pc_$(NAME).o: pc_$(NAME).hip pc_$(NAME).h ../../include/pcodec.h $(SHARED) $(EXTRA_DEPS)
	$(HIPCC) $(FLAGS) -I../../include -I../image_csrc -c $< -o $@

$(OUT): pc_$(NAME).o
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC $< -o $@

clean:
	rm -f pc_$(NAME).o $(OUT)

.PHONY: all clean
