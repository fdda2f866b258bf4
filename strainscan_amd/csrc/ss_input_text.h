// An input file as one text in host memory, for the callers that walk a file's records in file order: ss_extract_write
// (ss_extract.hip) and ss_reads_load_pairs (ss_pairs.hip).  Host code only, no HIP: tests/extract_fuzz.cpp compiles it with g++.
#pragma once
#include <fcntl.h>
#include <stdint.h>
#include <stdlib.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>

#include "strainscan_hip.h"

namespace ss {
// (ss_host.hip, ss_ingest.hip; the values of input_kind are those of ss_input_kind)
int min_base_qual();
int input_kind(const char *path);
bool inflate_whole(const char *path, uint64_t budget, char **text, uint64_t *len, int mode, unsigned threads);
uint64_t inflate_budget_bytes();

// an input file as one text in memory: a plain file mapped, a .gz inflated whole
struct InputText {
    const char *p = nullptr;
    uint64_t n = 0;
    void *map = nullptr;
    uint64_t map_n = 0;
    char *owned = nullptr;
    ~InputText()
    {
        if (map) munmap(map, map_n);
        free(owned);
    }
    int open_path(const char *path)
    {
        if (!path || !path[0]) return SS_EINVAL;
        const int kind = ss::input_kind(path);
        if (kind == 1 || kind == 2 || kind == 3) return SS_EINVAL;      // BAM, CRAM: not extracted from
        if (kind == 4) {
            if (ss::inflate_whole(path, ss::inflate_budget_bytes(), &owned, &n, 0, 0)) { p = owned; return SS_OK; }
            owned = nullptr;
            return inflate_zlib(path);
        }
        const int fd = open(path, O_RDONLY);
        if (fd < 0) return SS_EIO;
        struct stat st;
        if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode)) { close(fd); return SS_EIO; }
        n = (uint64_t)st.st_size;
        if (n) {
            void *m = mmap(nullptr, n, PROT_READ, MAP_PRIVATE, fd, 0);
            if (m == MAP_FAILED) { close(fd); n = 0; return SS_EIO; }
            map = m;
            map_n = n;
            p = (const char *)m;
        }
        close(fd);
        return SS_OK;
    }
    int inflate_zlib(const char *path)
    {
        gzFile f = gzopen(path, "rb");
        if (!f) return SS_EIO;
        gzbuffer(f, 1 << 20);
        uint64_t cap = 1 << 22, got = 0;
        char *buf = (char *)malloc(cap);
        int rc = buf ? SS_OK : SS_ENOMEM;
        while (rc == SS_OK) {
            if (got == cap) {
                char *nb = (char *)realloc(buf, cap * 2);
                if (!nb) { rc = SS_ENOMEM; break; }
                buf = nb;
                cap *= 2;
            }
            const int r = gzread(f, buf + got, (unsigned)std::min<uint64_t>(cap - got, 1u << 30));
            if (r < 0) { rc = SS_EIO; break; }
            if (r == 0) break;
            got += (uint64_t)r;
        }
        gzclose(f);
        if (rc != SS_OK) { free(buf); return rc; }
        owned = buf;
        p = buf;
        n = got;
        return SS_OK;
    }
};

}  // namespace ss
